"""The two-phase system proof on the GPU: the range transpose and commitment
(mlh_trace_columns_range, mlh_trace_commit_range), the sumcheck with sum
columns (mlh_cs_sumcheck_prove_sums), mlh_field_inv and the composed proof
(mlh_system_prove_phased, multilinear_amd.constraint_system) against the
plain-Python model tests/phased_reference.py.  Every comparison is bit-exact."""
import ctypes
import random

import numpy as np
import pytest
import torch

import cs_cases
import phased_reference as PR
import system_reference as S
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.batched import BatchedPCSProof
from multilinear_amd.polynomials import eq_table
from multilinear_amd.transcript import Transcript
from oracle import field as F

pytestmark = pytest.mark.gpu

M = F.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]
VERIFY = _lib.STATUS_CODES["MLH_ERR_VERIFY"]


def _dev(values):
    return D.to_device(D.ints_to_limbs(values))


def _host(t):
    return D.limbs_to_ints(D.from_device(t))


def _start(mo):
    tr = Transcript()
    tr.absorb(mo["seed"])
    return tr


# ---- mlh_trace_columns_range ----------------------------------------------------

def _range_info(log_height, width, col0, ncols):
    rows, blocks = ctypes.c_uint32(), ctypes.c_uint32()
    assert D.lib().mlh_trace_columns_range_launch_info(log_height, width, col0, ncols,
                                                       ctypes.byref(rows), ctypes.byref(blocks)) == 0
    return rows.value, blocks.value


# (0, 3, 1, 2), (1, 4, 0, 1): below one tile; (5, 7, 3, 4): odd width, even range; (9, 32, 5, 22):
# the pitch rule's "W >= 8, even" case off a 16-byte-odd start; (9, 32, 31, 1): 16-byte runs;
# (11, 6, 1, 5): odd range over several tiles; (13, 4, 2, 2): several tiles, one per block
RANGES = [(0, 3, 1, 2), (1, 4, 0, 1), (5, 7, 3, 4), (9, 32, 5, 22), (9, 32, 31, 1), (11, 6, 1, 5),
          (13, 4, 2, 2)]


@pytest.mark.parametrize("log_height,width,col0,ncols", RANGES)
def test_range_transpose_is_the_slice(log_height, width, col0, ncols):
    h = 1 << log_height
    a = D.random_limbs(h * width, seed=100000 * log_height + 1000 * width + 32 * col0 + ncols)
    m = D.to_device(a)
    out = CS.trace_columns(m, width, columns=(col0, ncols))
    want = a.reshape(h, width, 4)[:, col0:col0 + ncols].transpose(1, 0, 2).reshape(-1, 4)
    assert np.array_equal(D.from_device(out), want)
    assert np.array_equal(D.from_device(m), a)  # out of place: the input is unchanged
    rows, blocks = _range_info(log_height, width, col0, ncols)
    assert blocks == max(1, h // rows)  # none of these reaches the grid cap
    # the out-of-range columns filled with a second pattern: the same output
    b = D.random_limbs(h * width, seed=7).reshape(h, width, 4)
    b[:, col0:col0 + ncols] = a.reshape(h, width, 4)[:, col0:col0 + ncols]
    out2 = CS.trace_columns(D.to_device(b.reshape(-1, 4)), width, columns=(col0, ncols))
    assert torch.equal(out, out2)


@pytest.mark.parametrize("log_height,width", [(5, 7), (11, 6)])
def test_range_over_the_whole_width_is_trace_columns(log_height, width):
    """col0 = 0, ncols = width runs the contiguous kernel: mlh_trace_columns'
    bytes and launch shape.  (5, 7): one short tile; (11, 6): several tiles of
    an odd-pitch width."""
    m = D.random_device((1 << log_height) * width, seed=1000 * log_height + width)
    out = CS.trace_columns(m, width, columns=(0, width))
    assert torch.equal(out, CS.trace_columns(m, width))
    rows, blocks = ctypes.c_uint32(), ctypes.c_uint32()
    assert D.lib().mlh_trace_columns_launch_info(log_height, width, ctypes.byref(rows),
                                                 ctypes.byref(blocks)) == 0
    assert _range_info(log_height, width, 0, width) == (rows.value, blocks.value)


def test_range_transpose_block_takes_a_second_tile():
    """The smallest shape at which a block loops: the grid caps at 1024 blocks
    and the tile has at least 64 rows (ncols = 31: 64 x 31 <= 2048 < 128 x 31),
    so 2^17 rows."""
    width, col0, ncols = 32, 1, 31
    log_height = next(L for L in range(1, 33)
                      if (1 << L) // _range_info(L, width, col0, ncols)[0]
                      > _range_info(L, width, col0, ncols)[1])
    rows, blocks = _range_info(log_height, width, col0, ncols)
    print("range transpose 2^%d x %d [%d, +%d): %d tiles of %d rows on %d blocks"
          % (log_height, width, col0, ncols, (1 << log_height) // rows, rows, blocks))
    assert log_height == 17
    h = 1 << log_height
    m = D.random_device(h * width, seed=17)
    out = CS.trace_columns(m, width, columns=(col0, ncols))
    assert torch.equal(out.view(ncols, h, 4), m.view(h, width, 4)[:, col0:].permute(1, 0, 2))


def test_range_transpose_argument_errors():
    lib, ctx = D.lib(), D.context()
    m, out = D.empty(64), D.empty(64)
    f = lib.mlh_trace_columns_range
    assert f(ctx, D.ptr(m), 3, 4, 0, 0, D.ptr(out)) == INVALID   # no columns
    assert f(ctx, D.ptr(m), 3, 4, 4, 1, D.ptr(out)) == INVALID   # starts past the trace
    assert f(ctx, D.ptr(m), 3, 4, 2, 3, D.ptr(out)) == INVALID   # leaves the trace
    assert f(ctx, D.ptr(m), 3, 4, 1, 0xFFFFFFFF, D.ptr(out)) == INVALID
    assert f(ctx, None, 3, 4, 1, 2, D.ptr(out)) == INVALID
    assert f(ctx, D.ptr(m), 3, 4, 1, 2, None) == INVALID
    assert f(ctx, D.ptr(m), 3, 4, 1, 2, D.ptr(m)) == INVALID     # in place
    assert f(ctx, D.ptr(m), 3, 4, 1, 2, D.ptr(out)) == 0


# ---- mlh_trace_commit_range -----------------------------------------------------

def _commit(m, log_height, width, col0=None, ncols=None):
    h = ctypes.c_void_p()
    if col0 is None:
        st = D.lib().mlh_trace_commit(D.context(), D.ptr(m), log_height, width, ctypes.byref(h))
    else:
        st = D.lib().mlh_trace_commit_range(D.context(), D.ptr(m), log_height, width, col0, ncols,
                                            ctypes.byref(h))
    return st, h


def _root(h):
    out = (ctypes.c_uint8 * 32)()
    assert D.lib().mlh_trace_commitment_root(h, out) == 0
    return bytes(out)


@pytest.mark.parametrize("name", PR.NAMES)
def test_commit_range_roots(name):
    mo = PR.model(name)
    L, W, P = mo["log_height"], mo["width"], mo["pre"]
    lib = D.lib()
    m = _dev(mo["matrix"])
    handles = []
    try:
        st, h1 = _commit(m, L, W, 0, P)
        assert st == 0, lib.mlh_last_error(D.context())
        handles.append(h1)
        assert lib.mlh_trace_commitment_width(h1) == P
        assert lib.mlh_trace_commitment_log_height(h1) == L
        assert _root(h1) == mo["root1"]
        if P < W:
            st, h2 = _commit(m, L, W, P, W - P)
            assert st == 0
            handles.append(h2)
            assert lib.mlh_trace_commitment_width(h2) == W - P
            assert _root(h2) == mo["root2"]
        assert _host(m) == mo["matrix"]
        # the batch commitment of the batched PCS over those columns
        cols = CS.trace_columns(m, W, columns=(0, P))
        pr = BatchedPCSProof.prove(mo["rs"], mo["output"][:P], cols, Transcript())
        assert pr.fri_proof.batch_commitment == mo["root1"]
        # the (0, W) range is mlh_trace_commit's root
        st, hf = _commit(m, L, W)
        assert st == 0
        handles.append(hf)
        st, hr = _commit(m, L, W, 0, W)
        assert st == 0
        handles.append(hr)
        assert _root(hf) == _root(hr)
        # root1 does not depend on the columns at and above P
        if P < W:
            m.view(1 << L, W, 4)[:, P:] = 0x5A5A5A5
            st, h3 = _commit(m, L, W, 0, P)
            assert st == 0
            handles.append(h3)
            assert _root(h3) == mo["root1"]
    finally:
        for h in handles:
            lib.mlh_trace_commitment_destroy(h)


def test_commit_range_argument_errors():
    m = _dev(list(range(24)))
    for col0, ncols in ((0, 0), (3, 1), (1, 3)):  # P = 0 among them
        st, h = _commit(m, 3, 3, col0, ncols)
        assert st == INVALID and not h.value
    st, h = _commit(m, 0, 3, 0, 1)
    assert st == INVALID and not h.value


# ---- mlh_cs_sumcheck_prove_sums -------------------------------------------------

def _prove_sums(name, mo, mask, beta, claim, plain=False):
    """The rounds on the model's pre-sumcheck transcript -> (polys, rs, folded matrix, digest)."""
    lib, ctx = D.lib(), D.context()
    prog = CS.Program(S.program_wire(name))
    L, W, Dg = mo["log_height"], mo["width"], mo["degree"] + 1
    ch = mo["sysm"].challenges
    m = _dev(mo["matrix"])
    delta = eq_table(ch.row)
    tr = _start(mo)
    tr.absorb(mo["root1"])
    if mo["root2"] is not None:
        tr.absorb(mo["root2"])
    if mo["sum_columns"]:
        tr.absorb(F.to_bytes(mo["column_sum"]))
    assert tr.random() == mo["before_sumcheck"].random()
    polys = (ctypes.c_uint8 * (16 * Dg * L))()
    rs = (ctypes.c_uint8 * (16 * L))()
    if plain:
        st = lib.mlh_cs_sumcheck_prove(ctx, prog.h, W, D.ptr(m), D.ptr(delta), L, CS._elems(ch.trace),
                                       CS._elems(mo["sysm"].constraint_mask), D.fe_bytes(claim), tr.h,
                                       polys, rs)
    else:
        st = lib.mlh_cs_sumcheck_prove_sums(ctx, prog.h, W, D.ptr(m), D.ptr(delta), L,
                                            CS._elems(ch.trace),
                                            CS._elems(mo["sysm"].constraint_mask), mask,
                                            None if beta is None else D.fe_bytes(beta),
                                            D.fe_bytes(claim), tr.h, polys, rs)
    assert st == 0, lib.mlh_last_error(ctx)
    return bytes(polys), bytes(rs), _host(m), tr.random()


@pytest.mark.parametrize("name", PR.NAMES)
def test_prove_sums_matches_model(name):
    mo = PR.model(name)
    L, W, Dg = mo["log_height"], mo["width"], mo["degree"] + 1
    polys, rs, folded, digest = _prove_sums(name, mo, mo["mask"], mo["beta"], mo["claim"])
    flat = CS._split(polys, Dg * L)
    assert [flat[Dg * k:Dg * k + Dg] for k in range(L)] == mo["pols"]
    assert CS._split(rs, L) == mo["rs"]
    assert folded[:W] == mo["output"]
    assert digest == mo["after_sumcheck"]


@pytest.mark.parametrize("name", ["lin1", "deg5_w7", "cubic4"])
def test_prove_sums_mask_zero_is_the_plain_prover(name):
    mo = PR.model(name)
    a = _prove_sums(name, mo, 0, None, mo["total"])
    b = _prove_sums(name, mo, 0, None, mo["total"], plain=True)
    assert a == b
    c = _prove_sums(name, mo, 0, mo["beta"], mo["total"])  # beta is not read
    assert a == c


# ---- mlh_system_prove_phased ----------------------------------------------------

def _prove(name, mo, tr, matrix1=None, mask=None, prog=None, com1="range", com2="range",
           null=None):
    """-> (status, PhasedSystemProof buffers, the folded matrix tensor)."""
    lib, ctx = D.lib(), D.context()
    L, W, P = mo["log_height"], mo["width"], mo["pre"]
    prog = prog or CS.Program(S.program_wire(name))
    work = _dev(mo["matrix"])
    handles = []

    def make(kind, col0, ncols):
        if kind is None or (kind == "range" and ncols == 0):
            return None
        if kind == "full":
            col0, ncols = 0, W
        src = _dev(matrix1) if (matrix1 is not None and col0 == 0) else work
        st, h = _commit(src, L, W, col0, ncols)
        assert st == 0
        handles.append(h)
        return h

    h1 = make(com1, 0, P)
    h2 = make(com2, P, W - P)
    p = CS.PhasedSystemProof(L, W, mo["degree"], P, mo["mask"])
    args = dict(sum=D.fe_bytes(mo["total"]), column_sum=D.fe_bytes(mo["column_sum"]), tr=tr.h,
                proof=ctypes.byref(p.c), matrix=D.ptr(work))
    if null:
        args[null] = None
    try:
        st = lib.mlh_system_prove_phased(ctx, prog.h, h1, h2, mo["mask"] if mask is None else mask,
                                         args["matrix"], args["sum"], args["column_sum"], args["tr"],
                                         args["proof"])
    finally:
        for h in handles:
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


def _verify(name, mo, p, tr):
    prog = CS.Program(S.program_wire(name))
    return D.lib().mlh_system_verify_phased(prog.h, mo["log_height"], mo["pre"], mo["mask"],
                                            D.fe_bytes(mo["total"]), D.fe_bytes(mo["column_sum"]),
                                            ctypes.byref(p.c), tr.h)


@pytest.mark.parametrize("name", PR.NAMES)
def test_prove_matches_model_and_verifies(name):
    mo = PR.model(name)
    tr = _start(mo)
    entry = tr.clone()
    st, p, work = _prove(name, mo, tr)
    assert st == 0, D.lib().mlh_last_error(D.context())
    assert (p.c.log_height, p.c.width, p.c.degree, p.c.pre_random_columns, p.c.sum_column_mask) == \
        (mo["log_height"], mo["width"], mo["degree"], mo["pre"], mo["mask"])
    assert p.sumcheck_polynomials == mo["pols"]
    assert p.output == mo["output"]
    assert _host(work)[:mo["width"]] == mo["output"]  # row 0 of the folded matrix
    assert len(p.pcs) == len(mo["pcs"])
    for got, want in zip(p.pcs, mo["pcs"]):
        _assert_pcs_equals_model(got, want)
    assert tr.random() == mo["digest"]
    assert _verify(name, mo, p, entry) == 0
    assert entry.random() == mo["digest"]


@pytest.mark.parametrize("name", PR.NAMES)
def test_openings_equal_standalone_batched_pcs(name):
    """Each opening is byte-identical to mlh_batched_pcs_prove on its columns,
    run on a transcript that absorbed the same bytes."""
    mo = PR.model(name)
    L, W, P = mo["log_height"], mo["width"], mo["pre"]
    tr = _start(mo)
    st, p, _ = _prove(name, mo, tr)
    assert st == 0
    t2 = _start(mo)
    for root in p.commitments:
        t2.absorb(root)
    if mo["sum_columns"]:
        t2.absorb(F.to_bytes(mo["column_sum"]))
    for pol in p.sumcheck_polynomials:
        for c in pol:
            t2.absorb(F.to_bytes(c))
    assert t2.random() == mo["after_sumcheck"]
    m = _dev(mo["matrix"])
    ranges = [(0, P)] + ([(P, W - P)] if P < W else [])
    for (col0, ncols), got in zip(ranges, p.pcs):  # t2 runs on through both
        cols = CS.trace_columns(m, W, columns=(col0, ncols))
        alone = BatchedPCSProof.prove(mo["rs"], p.output[col0:col0 + ncols], cols, t2)
        assert bytes(alone.fri_proof.c.batch_commitment) == bytes(got.c.fri.batch_commitment)
        assert bytes(alone.fri_proof._commit) == bytes(got.fri_proof._commit)
        assert bytes(alone._polys) == bytes(got._polys)
        assert alone.fri_proof.last_elem == got.fri_proof.last_elem
        assert alone.fri_proof.last_random == got.fri_proof.last_random
        assert alone.fri_proof.query_indices == got.fri_proof.query_indices
        assert bytes(alone.fri_proof._q) == bytes(got.fri_proof._q)
    assert t2.random() == tr.random()


def test_one_phase_no_sums_is_mlh_system_prove():
    name = "pythagorean"
    mo = PR.model(name)
    assert mo["pre"] == mo["width"] and mo["mask"] == 0
    tr = _start(mo)
    st, p, _ = _prove(name, mo, tr, com1="full", com2=None)  # mlh_trace_commit's own handle
    assert st == 0
    lib, ctx = D.lib(), D.context()
    L, W = mo["log_height"], mo["width"]
    prog = CS.Program(S.program_wire(name))
    m = _dev(mo["matrix"])
    st, h = _commit(m, L, W)
    assert st == 0
    q = CS.SystemProof(L, W, mo["degree"])
    t2 = _start(mo)
    try:
        assert lib.mlh_system_prove(ctx, prog.h, h, D.ptr(m), D.fe_bytes(mo["total"]), t2.h,
                                    ctypes.byref(q.c)) == 0
    finally:
        lib.mlh_trace_commitment_destroy(h)
    q._sync()
    assert bytes(p._polys) == bytes(q._polys) and bytes(p._output) == bytes(q._output)
    a, b = p.pcs[0], q.pcs
    assert bytes(a.c.fri.batch_commitment) == bytes(b.c.fri.batch_commitment)
    assert bytes(a.fri_proof._commit) == bytes(b.fri_proof._commit)
    assert bytes(a._polys) == bytes(b._polys)
    assert a.fri_proof.last_elem == b.fri_proof.last_elem
    assert a.fri_proof.last_random == b.fri_proof.last_random
    assert a.fri_proof.query_indices == b.fri_proof.query_indices
    assert bytes(a.fri_proof._q) == bytes(b.fri_proof._q)
    assert tr.random() == t2.random() == S.model(name)["digest"]


def test_trace_changed_after_commitment_1_proves_but_does_not_verify():
    name = "deg5_w7"
    mo = PR.model(name)
    W = mo["width"]
    committed = list(mo["matrix"])
    committed[3 * W + 1] = (committed[3 * W + 1] + 1) % M  # column 1 < P = 4
    tr = _start(mo)
    entry = tr.clone()
    st, p, _ = _prove(name, mo, tr, matrix1=committed)
    assert st == 0
    assert _verify(name, mo, p, entry) == VERIFY
    assert entry.random() == mo["entry"]


@pytest.mark.parametrize("what", ["width_mismatch", "com2_with_P_equal_W", "com2_missing",
                                  "null_com1_P_0", "null_proof", "null_sum", "null_column_sum",
                                  "null_matrix", "mask_bit_at_W"])
def test_prove_argument_errors_leave_transcript_unchanged(what):
    name = "quad3"  # W = 3, P = 1
    mo = PR.model(name)
    tr = _start(mo)
    kw = {"width_mismatch": dict(prog=CS.Program(S.program_wire("pythagorean"))),
          "com2_with_P_equal_W": dict(com1="full"),
          "com2_missing": dict(com2=None),
          "null_com1_P_0": dict(com1=None, com2="full"),
          "null_proof": dict(null="proof"), "null_sum": dict(null="sum"),
          "null_column_sum": dict(null="column_sum"), "null_matrix": dict(null="matrix"),
          "mask_bit_at_W": dict(mask=mo["mask"] | (1 << mo["width"]))}[what]
    st, _, work = _prove(name, mo, tr, **kw)
    assert st == INVALID
    assert tr.random() == mo["entry"]
    assert _host(work) == mo["matrix"]


# ---- mlh_field_inv --------------------------------------------------------------

def _inv_want(vals):
    return [pow(v, M - 2, M) for v in vals]


@pytest.mark.parametrize("n", [1, 63, 64, 255, 257, (1 << 12) + 3, 5 * 4096 + 1234])
def test_field_inv_matches_fermat(n):
    r = random.Random(n)
    vals = [r.randrange(M) for _ in range(n)]
    for i, v in zip(range(0, n, 7), (0, 1, M - 1, 2, 0)):
        vals[i] = v
    # zeros straddling one thread's elements (stride 256) and its neighbours
    for i in (256, 257, 512, 768 + 1, 1023, 1024):
        if i < n:
            vals[i] = 0
    a = _dev(vals)
    out = CS.field_inv(a)
    assert _host(out) == _inv_want(vals)
    assert _host(a) == vals
    got = CS.field_inv(a, out=a)  # in place
    assert got is a and _host(a) == _inv_want(vals)


def test_field_inv_zero_runs():
    n = 3 * 8192 + 77
    r = random.Random(5)
    vals = [r.randrange(1, M) for _ in range(n)]
    # every element of thread 3 of block 0 under any K <= 32, i.e. one whole
    # chunk of zeros: 3, 3 + 256, ...; and a contiguous run over block borders
    for k in range(32):
        vals[3 + 256 * k] = 0
    for i in range(8192 - 300, 8192 + 300):
        vals[i] = 0
    out = CS.field_inv(_dev(vals))
    assert _host(out) == _inv_want(vals)
    z = D.to_device(np.zeros((4099, 4), dtype=np.uint32))
    assert not D.from_device(CS.field_inv(z)).any()  # all zeros


def test_field_inv_times_input_is_one_and_edges():
    lib, ctx = D.lib(), D.context()
    n = 20000
    a = D.random_device(n, seed=3)
    inv = CS.field_inv(a)
    prod = CS.field_mul(a, inv)
    nz = (a != 0).any(dim=1)
    one = torch.zeros_like(prod)
    one[:, 0] = 1
    assert torch.equal(prod[nz], one[nz])
    assert int(nz.sum()) >= n - 1
    # n = 0 is a no-op, null pointers allowed then
    assert lib.mlh_field_inv(ctx, None, None, 0) == 0
    assert lib.mlh_field_inv(ctx, D.ptr(a), None, 4) == INVALID
    assert lib.mlh_field_inv(ctx, None, D.ptr(a), 4) == INVALID
    shifted = ctypes.c_void_p(a.data_ptr() + 16)  # overlapping, not in place
    assert lib.mlh_field_inv(ctx, D.ptr(a), shifted, 8) == INVALID


# ---- a lookup, end to end, with the columns filled on the device -----------------

LOOKUP_L = 6
COL_A, COL_T, COL_M, COL_U, COL_V = range(5)


def _lookup_inputs(bump=False):
    """2^6 rows: a = values looked up, t = the table (distinct), m = how often
    t[i] occurs in a.  Fixed small integers."""
    h = 1 << LOOKUP_L
    t = [3 * i + 2 for i in range(h)]
    r = random.Random("lookup")
    a = [t[r.randrange(16)] for _ in range(h)]
    m = [a.count(x) for x in t]
    if bump:
        m[5] += 1
    return a, t, m


def _lookup_system():
    cset = CS.ConstraintSet([CS.var(COL_U) * (CS.rand(0) - CS.var(COL_A)) - 1,
                             CS.var(COL_V) * (CS.rand(0) - CS.var(COL_T)) + CS.var(COL_M)], 2)
    layout = CS.WitnessLayout(columns=5, randoms=1, pre_random_columns=3,
                              sum_columns=(COL_U, COL_V))
    return cset, layout


def _lookup_prove(bump):
    h = 1 << LOOKUP_L
    a, t, m = _lookup_inputs(bump)
    rows = [[a[i], t[i], m[i], 0, 0] for i in range(h)]
    matrix = _dev([v for row in rows for v in row])
    cset, layout = _lookup_system()
    trace = CS.Trace(matrix, 5)
    tr = Transcript()
    tr.absorb(b"lookup")
    vt = tr.clone()
    prover = CS.System.phased_prover(tr, cset, layout, trace)
    gamma = prover.randoms[0]
    assert all((gamma - x) % M for x in a + t)  # no zero denominator for this seed
    # u = 1 / (gamma - a), v = -m / (gamma - t), on the device
    mv = matrix.view(h, 5, 4)
    col = lambda j: mv[:, j].contiguous()
    g = _dev([gamma] * h)
    u = CS.field_inv(CS.field_sub(g, col(COL_A)))
    v = CS.field_mul(CS.field_scale(col(COL_M), M - 1), CS.field_inv(CS.field_sub(g, col(COL_T))))
    mv[:, COL_U] = u  # torch strided copies into the matrix
    mv[:, COL_V] = v
    want_u = [pow((gamma - x) % M, M - 2, M) for x in a]
    want_v = [(-mi * pow((gamma - x) % M, M - 2, M)) % M for mi, x in zip(m, t)]
    assert _host(u) == want_u and _host(v) == want_v
    proof = prover.prove(tr, 0, 0)
    return proof, vt, cset, layout, (sum(want_u) + sum(want_v)) % M


def test_lookup_verifies_and_a_wrong_multiplicity_does_not():
    proof, vt, cset, layout, colsum = _lookup_prove(bump=False)
    assert colsum == 0  # sum_i 1/(g - a_i) = sum_i m_i/(g - t_i)
    entry = vt.random()
    assert proof.verify(vt, cset, layout, 0, 0)
    assert vt.random() != entry
    bad, vt2, cset, layout, colsum2 = _lookup_prove(bump=True)
    assert colsum2 != 0
    entry2 = vt2.random()
    assert not bad.verify(vt2, cset, layout, 0, 0)
    assert vt2.random() == entry2


# ---- Python mirror -------------------------------------------------------------------

def test_python_mirror_round_trip():
    name = "deg5_w7"
    mo = PR.model(name)
    c = S.CASES[name]
    exprs = [CS.var(0) * CS.var(1) * CS.var(2) * CS.var(3) - CS.var(4),
             CS.var(5) * CS.var(6) - CS.rand(0),
             CS.var(0) - CS.var(6) * 3,
             -(CS.var(1) * CS.var(1)) + CS.rand(1) * CS.var(2),
             CS.var(3)]
    assert CS.compile_program(exprs, 7, 2, 5) == c.wire
    cset = CS.ConstraintSet(exprs, 5)
    layout = CS.WitnessLayout(columns=7, randoms=2, pre_random_columns=mo["pre"],
                              sum_columns=mo["sum_columns"])
    trace = CS.Trace(_dev(mo["matrix"]), 7)
    tr = _start(mo)
    vt = tr.clone()
    prover = CS.System.phased_prover(tr, cset, layout, trace)
    assert tr.random() == mo["entry"]  # the roots are absorbed by prove
    assert prover.commitment().root() == mo["root1"]
    assert prover.randoms == mo["trace_randoms"]
    proof = prover.prove(tr, mo["total"], mo["column_sum"])
    assert _host(trace.matrix()) == mo["matrix"]  # prove folds a clone
    assert tr.random() == mo["digest"]
    assert proof.commitments == [mo["root1"], mo["root2"]]
    assert proof.sumcheck_polynomials == mo["pols"] and proof.output == mo["output"]
    assert proof.verify(vt, cset, layout, mo["total"], mo["column_sum"])
    assert vt.random() == mo["digest"]
    bad = _start(mo)
    assert not proof.verify(bad, cset, layout, mo["total"], (mo["column_sum"] + 1) % M)
    assert bad.random() == mo["entry"]
    # the same bytes as the C ABI path
    st, p, _ = _prove(name, mo, _start(mo))
    assert st == 0
    assert bytes(proof._polys) == bytes(p._polys) and bytes(proof._output) == bytes(p._output)
    for a, b in zip(proof.pcs, p.pcs):
        assert bytes(a._polys) == bytes(b._polys)
        assert bytes(a.fri_proof._commit) == bytes(b.fri_proof._commit)
        assert bytes(a.fri_proof._q) == bytes(b.fri_proof._q)
        assert a.fri_proof.last_random == b.fri_proof.last_random
