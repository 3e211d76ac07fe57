"""Trace commitment and system proof on the GPU (mlh_trace_columns,
mlh_trace_commit, mlh_system_prove through the C ABI and
multilinear_amd.constraint_system) against the plain-Python model
tests/system_reference.py.  Every comparison is bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import cs_cases
import system_reference as S
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.batched import BatchedPCSProof
from multilinear_amd.transcript import Transcript
from oracle import field as F

pytestmark = pytest.mark.gpu

INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]
VERIFY = _lib.STATUS_CODES["MLH_ERR_VERIFY"]
COMMIT_NAMES = ["lin1", "quad3", "deg5_w7", "wide32", "cubic4"]
PROVE_NAMES = ["pythagorean"] + COMMIT_NAMES


def _dev(values):
    return D.to_device(D.ints_to_limbs(values))


def _host(t):
    return D.limbs_to_ints(D.from_device(t))


def _start(mo):
    tr = Transcript()
    tr.absorb(mo["seed"])
    return tr


def _launch_info(log_height, width):
    rows, blocks = ctypes.c_uint32(), ctypes.c_uint32()
    assert D.lib().mlh_trace_columns_launch_info(log_height, width, ctypes.byref(rows),
                                                 ctypes.byref(blocks)) == 0
    return rows.value, blocks.value


# ---- mlh_trace_columns -----------------------------------------------------------

# (0, 1), (0, 5), (1, 1), (3, 1): below one tile; (5, 7): W not a power of two;
# (9, 32): the widest; (10, 3): odd width over several tiles; (13, 4): 16 tiles
# of 512 rows, one per block.  The grid caps at 1024 blocks, which no table of
# width 4 below 2^20 rows reaches; the shape that loops is (17, 32): 2048 tiles
# of 64 rows, two per block (test_trace_columns_block_loops_over_tiles).
SHAPES = [(0, 1), (0, 5), (1, 1), (3, 1), (5, 7), (9, 32), (10, 3), (13, 4)]


@pytest.mark.parametrize("log_height,width", SHAPES)
def test_trace_columns_is_the_transpose(log_height, width):
    h = 1 << log_height
    a = D.random_limbs(h * width, seed=1000 * log_height + width)
    m = D.to_device(a)
    out = CS.trace_columns(m, width)
    want = a.reshape(h, width, 4).transpose(1, 0, 2).reshape(-1, 4)
    assert np.array_equal(D.from_device(out), want)
    assert np.array_equal(D.from_device(m), a)  # out of place: the input is unchanged
    rows, blocks = _launch_info(log_height, width)
    assert blocks == max(1, h // rows)  # none of these reaches the grid cap


def test_trace_columns_block_loops_over_tiles():
    log_height, width = 17, 32
    rows, blocks = _launch_info(log_height, width)
    tiles = (1 << log_height) // rows
    print("trace_columns 2^%d x %d: %d tiles of %d rows on %d blocks" % (log_height, width, tiles,
                                                                       rows, blocks))
    assert tiles > blocks  # a block takes more than one tile
    h = 1 << log_height
    m = D.random_device(h * width, seed=17)
    keep = m.clone()
    out = CS.trace_columns(m, width)
    assert torch.equal(out.view(width, h, 4), m.view(h, width, 4).permute(1, 0, 2))
    assert torch.equal(m, keep)


def test_trace_columns_argument_errors():
    lib, ctx = D.lib(), D.context()
    m, out = D.empty(64), D.empty(64)
    assert lib.mlh_trace_columns(ctx, D.ptr(m), 3, 0, D.ptr(out)) == INVALID
    assert lib.mlh_trace_columns(ctx, D.ptr(m), 1, 33, D.ptr(out)) == INVALID
    assert lib.mlh_trace_columns(ctx, None, 3, 4, D.ptr(out)) == INVALID
    assert lib.mlh_trace_columns(ctx, D.ptr(m), 3, 4, None) == INVALID
    assert lib.mlh_trace_columns(None, D.ptr(m), 3, 4, D.ptr(out)) == INVALID
    assert lib.mlh_trace_columns(ctx, D.ptr(m), 3, 4, D.ptr(m)) == INVALID  # in place
    tail = ctypes.c_void_p(m.data_ptr() + 16 * 31)  # the last element overlaps
    assert lib.mlh_trace_columns(ctx, D.ptr(m), 3, 4, tail) == INVALID
    assert lib.mlh_trace_columns(ctx, D.ptr(m), 3, 4, D.ptr(out)) == 0


# ---- commit ------------------------------------------------------------------------

def _commit(m, log_height, width):
    h = ctypes.c_void_p()
    st = D.lib().mlh_trace_commit(D.context(), D.ptr(m), log_height, width, ctypes.byref(h))
    return st, h


def _root(h):
    out = (ctypes.c_uint8 * 32)()
    assert D.lib().mlh_trace_commitment_root(h, out) == 0
    return bytes(out)


@pytest.mark.parametrize("name", COMMIT_NAMES)
def test_commit_root(name):
    mo = S.model(name)
    L, W = mo["log_height"], mo["width"]
    lib = D.lib()
    m = _dev(mo["matrix"])
    st, h = _commit(m, L, W)
    assert st == 0, lib.mlh_last_error(D.context())
    try:
        assert lib.mlh_trace_commitment_width(h) == W
        assert lib.mlh_trace_commitment_log_height(h) == L
        assert _root(h) == mo["root"]
        assert _host(m) == mo["matrix"]  # the handle does not change the trace
    finally:
        lib.mlh_trace_commitment_destroy(h)
    # the batch commitment of the batched PCS over mlh_trace_columns' output
    cols = CS.trace_columns(m, W)
    pr = BatchedPCSProof.prove(mo["rs"], mo["output"], cols, Transcript())
    assert pr.fri_proof.batch_commitment == mo["root"]


def test_commit_needs_one_variable():
    m = _dev([1, 2, 3])
    st, h = _commit(m, 0, 3)
    assert st == INVALID and not h.value
    st, h = _commit(m, 1, 0)
    assert st == INVALID and not h.value


# ---- prove -------------------------------------------------------------------------

def _prove(name, mo, tr, commit_matrix=None, prove_matrix=None, prog=None, null_proof=False):
    """-> (status, SystemProof buffers, the folded matrix tensor)."""
    lib, ctx = D.lib(), D.context()
    L, W = mo["log_height"], mo["width"]
    prog = prog or CS.Program(S.program_wire(name))
    cm = _dev(mo["matrix"] if commit_matrix is None else commit_matrix)
    st, h = _commit(cm, L, W)
    assert st == 0
    p = CS.SystemProof(L, W, mo["degree"])
    work = _dev(mo["matrix"] if prove_matrix is None else prove_matrix)
    try:
        st = lib.mlh_system_prove(ctx, prog.h, h, D.ptr(work), D.fe_bytes(mo["total"]), tr.h,
                                  None if null_proof else ctypes.byref(p.c))
    finally:
        lib.mlh_trace_commitment_destroy(h)
    p._sync()
    return st, p, work


def _assert_pcs_equals_model(pcs, want):
    fp = pcs.fri_proof
    assert fp.batch_commitment == want["batch_commitment"]
    assert fp.commitments == want["commitments"]
    assert pcs.sumcheck_polynomials == [tuple(p) for p in want["polys"]]
    assert fp.last_elem == want["last_elem"]
    assert fp.last_random == want["last_random"]
    assert fp.query_indices == want["indices"]
    assert bytes(fp._q) == want["queries"]


@pytest.mark.parametrize("name", PROVE_NAMES)
def test_prove_matches_model_and_verifies(name):
    mo = S.model(name)
    tr = _start(mo)
    entry = tr.clone()
    st, p, work = _prove(name, mo, tr)
    assert st == 0, D.lib().mlh_last_error(D.context())
    assert (p.c.log_height, p.c.width, p.c.degree) == (mo["log_height"], mo["width"], mo["degree"])
    assert p.sumcheck_polynomials == mo["pols"]
    assert p.output == mo["output"]
    assert _host(work)[:mo["width"]] == mo["output"]  # row 0 of the folded matrix
    _assert_pcs_equals_model(p.pcs, mo["pcs"])
    assert tr.random() == mo["digest"]
    prog = CS.Program(S.program_wire(name))
    assert D.lib().mlh_system_verify(prog.h, mo["log_height"], D.fe_bytes(mo["total"]),
                                     ctypes.byref(p.c), entry.h) == 0
    assert entry.random() == mo["digest"]


@pytest.mark.parametrize("name", PROVE_NAMES)
def test_pcs_part_equals_standalone_batched_pcs(name):
    """The opening is byte-identical to mlh_batched_pcs_prove on the columns
    at (rs, output), run on a transcript that absorbed the same bytes."""
    mo = S.model(name)
    tr = _start(mo)
    st, p, _ = _prove(name, mo, tr)
    assert st == 0
    t2 = _start(mo)
    t2.absorb(p.commitment)
    for pol in p.sumcheck_polynomials:
        for c in pol:
            t2.absorb(F.to_bytes(c))
    assert t2.random() == mo["after_sumcheck"]
    cols = CS.trace_columns(_dev(mo["matrix"]), mo["width"])
    alone = BatchedPCSProof.prove(mo["rs"], p.output, cols, t2)
    assert bytes(alone.fri_proof.c.batch_commitment) == p.commitment
    assert bytes(alone.fri_proof._commit) == bytes(p.pcs.fri_proof._commit)
    assert bytes(alone._polys) == bytes(p.pcs._polys)
    assert alone.fri_proof.last_elem == p.pcs.fri_proof.last_elem
    assert alone.fri_proof.last_random == p.pcs.fri_proof.last_random
    assert alone.fri_proof.query_indices == p.pcs.fri_proof.query_indices
    assert bytes(alone.fri_proof._q) == bytes(p.pcs.fri_proof._q)
    assert t2.random() == tr.random()


def test_wrong_trace_proves_but_does_not_verify():
    """The prover cannot tell that dev_matrix is not the committed trace: it
    returns a proof, and the verifier rejects it."""
    name = "deg5_w7"  # L = 5
    mo = S.model(name)
    other = list(mo["matrix"])
    other[3 * mo["width"] + 2] = (other[3 * mo["width"] + 2] + 1) % F.M
    tr = _start(mo)
    entry = tr.clone()
    st, p, _ = _prove(name, mo, tr, commit_matrix=mo["matrix"], prove_matrix=other)
    assert st == 0
    prog = CS.Program(S.program_wire(name))
    assert D.lib().mlh_system_verify(prog.h, mo["log_height"], D.fe_bytes(mo["total"]),
                                     ctypes.byref(p.c), entry.h) == VERIFY
    assert entry.random() == mo["entry"]


@pytest.mark.parametrize("what", ["width_mismatch", "null_proof"])
def test_prove_argument_errors_leave_transcript_unchanged(what):
    name = "quad3"
    mo = S.model(name)
    tr = _start(mo)
    kw = {"width_mismatch": dict(prog=CS.Program(S.program_wire("pythagorean"))),
          "null_proof": dict(null_proof=True)}[what]
    st, _, work = _prove(name, mo, tr, **kw)
    assert st == INVALID
    assert tr.random() == mo["entry"]
    assert _host(work) == mo["matrix"]


# ---- Python mirror -------------------------------------------------------------------

def test_python_mirror_round_trip():
    name = "pythagorean"
    mo = S.model(name)
    cset = CS.ConstraintSet(cs_cases.pythagorean_exprs(), 2)
    layout = CS.WitnessLayout(columns=4, randoms=0)
    trace = CS.Trace(_dev(mo["matrix"]), 4)
    tr = Transcript()
    vt = tr.clone()
    prover = CS.System.committed_prover(tr, cset, layout, trace)
    assert tr.random() == mo["entry"]  # the root is absorbed by prove
    assert prover.commitment().root() == mo["root"]
    assert prover.challenges().row() == mo["sysm"].challenges.row
    proof = prover.prove(tr, 0)
    assert _host(trace.matrix()) == mo["matrix"]  # prove folds a clone
    assert tr.random() == mo["digest"]
    assert proof.verify(vt, cset, layout, 0)
    assert vt.random() == mo["digest"]
    bad = Transcript()
    assert not proof.verify(bad, cset, layout, 1) and bad.random() == mo["entry"]
    # the same bytes as the C ABI path
    st, p, _ = _prove(name, mo, _start(mo))
    assert st == 0
    assert bytes(proof._polys) == bytes(p._polys) and bytes(proof._output) == bytes(p._output)
    assert proof.commitment == p.commitment
    assert bytes(proof.pcs._polys) == bytes(p.pcs._polys)
    assert bytes(proof.pcs.fri_proof._commit) == bytes(p.pcs.fri_proof._commit)
    assert bytes(proof.pcs.fri_proof._q) == bytes(p.pcs.fri_proof._q)
    assert proof.pcs.fri_proof.last_random == p.pcs.fri_proof.last_random
