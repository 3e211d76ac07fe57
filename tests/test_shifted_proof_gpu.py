"""Next-row constraints on the GPU: the row-rotated extension
(mlh_trace_extend_next), the rotated eq table (mlh_eq_table_rotate) and the
shifted system proof (mlh_system_prove_shifted, multilinear_amd's mirror)
against numpy and the plain-Python model tests/shifted_reference.py.  Every
comparison is bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import phased_reference as PR
import shifted_reference as SR
import system_reference as S
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.batched import BatchedPCSProof
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


def _u32(vals):
    return (ctypes.c_uint32 * max(len(vals), 1))(*vals)


# ---- mlh_trace_extend_next --------------------------------------------------------

def _extend_info(log_height, width, K):
    rows, blocks = ctypes.c_uint32(), ctypes.c_uint32()
    assert D.lib().mlh_trace_extend_next_launch_info(log_height, width, K, ctypes.byref(rows),
                                                     ctypes.byref(blocks)) == 0
    return rows.value, blocks.value


def _check_extend(log_height, width, cols, seed):
    H, K = 1 << log_height, len(cols)
    src = D.random_limbs(H * width, seed)
    T = np.ascontiguousarray(src).reshape(H, width, 4)
    want = np.concatenate([T, np.roll(T, -1, axis=0)[:, cols]], axis=1) if K else T
    m = D.to_device(src)
    before = m.clone()
    out = D.empty(H * (width + K))
    out.fill_(-1)
    D.check(D.lib().mlh_trace_extend_next(D.context(), D.ptr(m), log_height, width, _u32(cols), K,
                                          D.ptr(out)), D.context())
    got = D.from_device(out).reshape(H, width + K, 4)
    assert torch.equal(m, before)  # the source is not written
    assert np.array_equal(got, want)
    # the cells that read across a tile's edge, and the wrap to row 0
    rows, _ = _extend_info(log_height, width, K)
    for last in sorted(set(range(rows - 1, H, rows)) | {H - 1}):
        for k, c in enumerate(cols):
            assert np.array_equal(got[last, width + k], T[(last + 1) % H, c]), (last, k)
    return rows


@pytest.mark.parametrize("log_height,width,K", [(1, 1, 1), (2, 3, 2), (5, 7, 3), (9, 16, 16),
                                                (0, 2, 1), (7, 5, 0), (11, 4, 2)])
def test_extend_next_matches_numpy(log_height, width, K):
    cols = [(width - 1 - 2 * k) % width for k in range(K)]  # descending, wrapping: any order
    rows = _check_extend(log_height, width, cols, 40 + log_height)
    assert rows <= (1 << log_height)


def test_extend_next_block_loops_over_tiles():
    """The smallest height at which a block takes a second tile (W' = 17: tiles
    of 64 rows, 1088 elements)."""
    width, K = 9, 8
    log_height = next(L for L in range(33)
                      if ((1 << L) // _extend_info(L, width, K)[0]) > _extend_info(L, width, K)[1])
    rows, blocks = _extend_info(log_height, width, K)
    tiles = (1 << log_height) // rows
    print("extend_next 2^%d x %d + %d: %d tiles of %d rows on %d blocks" % (log_height, width, K,
                                                                            tiles, rows, blocks))
    assert tiles == 2 * blocks
    rows_lower, blocks_lower = _extend_info(log_height - 1, width, K)
    assert (1 << (log_height - 1)) // rows_lower == blocks_lower  # one tile per block below
    _check_extend(log_height, width, [8, 0, 3, 5, 1, 7, 2, 4], 77)


def test_extend_next_argument_errors():
    lib, ctx = D.lib(), D.context()
    m, out = D.empty(8 * 4), D.empty(8 * 6)
    cols = _u32([0, 3])
    f = lib.mlh_trace_extend_next
    assert f(ctx, D.ptr(m), 3, 4, cols, 2, D.ptr(out)) == 0
    assert f(None, D.ptr(m), 3, 4, cols, 2, D.ptr(out)) == INVALID
    assert f(ctx, None, 3, 4, cols, 2, D.ptr(out)) == INVALID
    assert f(ctx, D.ptr(m), 3, 4, cols, 2, None) == INVALID
    assert f(ctx, D.ptr(m), 3, 4, None, 2, D.ptr(out)) == INVALID
    assert f(ctx, D.ptr(m), 3, 4, _u32([0, 4]), 2, D.ptr(out)) == INVALID  # column at W
    assert f(ctx, D.ptr(m), 3, 0, cols, 2, D.ptr(out)) == INVALID
    assert f(ctx, D.ptr(m), 3, 31, cols, 2, D.ptr(out)) == INVALID  # W + K = 33
    assert f(ctx, D.ptr(m), 33, 4, cols, 2, D.ptr(out)) == INVALID
    assert f(ctx, D.ptr(m), 3, 4, cols, 2, D.ptr(m)) == INVALID  # in place
    tail = ctypes.c_void_p(m.data_ptr() + 16 * 31)
    assert f(ctx, D.ptr(m), 3, 4, cols, 2, tail) == INVALID
    rows, blocks = ctypes.c_uint32(), ctypes.c_uint32()
    g = lib.mlh_trace_extend_next_launch_info
    assert g(3, 31, 2, ctypes.byref(rows), ctypes.byref(blocks)) == INVALID
    assert g(3, 4, 2, None, ctypes.byref(blocks)) == INVALID


# ---- mlh_eq_table_rotate ------------------------------------------------------------

@pytest.mark.parametrize("log_n", [0, 1, 2, 12, 19])  # 19: 2048 blocks' worth on 1024 blocks
def test_eq_rotate_is_numpy_roll(log_n):
    src = D.random_limbs(1 << log_n, 90 + log_n)
    a = D.to_device(src)
    out = D.empty(1 << log_n)
    D.check(D.lib().mlh_eq_table_rotate(D.context(), D.ptr(a), log_n, D.ptr(out)), D.context())
    assert np.array_equal(D.from_device(out), np.roll(np.ascontiguousarray(src), 1, axis=0))
    assert np.array_equal(D.from_device(a), src)
    assert D.lib().mlh_eq_table_rotate(D.context(), D.ptr(a), log_n, D.ptr(a)) == INVALID


def test_eq_rotate_of_the_eq_table_is_the_successor_table():
    """rotate(eq(x))[j] = succ(x, j): the table against the closed form on
    0/1 points."""
    from multilinear_amd.polynomials import eq_table

    n, x = 4, [3, 5, 7, 11]
    out = D.empty(1 << n)
    D.check(D.lib().mlh_eq_table_rotate(D.context(), D.ptr(eq_table(x)), n, D.ptr(out)), D.context())
    got = _host(out)
    for j in range(1 << n):
        y = [(j >> (n - 1 - t)) & 1 for t in range(n)]
        r = (ctypes.c_uint8 * 16)()
        assert D.lib().mlh_shift_succ_evaluate(CS._elems(x), CS._elems(y), n, r) == 0
        assert got[j] == D.fe_from_bytes(r)


# ---- mlh_system_prove_shifted -------------------------------------------------------

def _commit(m, L, W, col0, ncols):
    h = ctypes.c_void_p()
    D.check(D.lib().mlh_trace_commit_range(D.context(), D.ptr(m), L, W, col0, ncols, ctypes.byref(h)),
            D.context())
    return h


def _prove(mo, wire, shifts, tr, matrix=None, committed=None, n_shifts=None, mask=None, null=None,
           drop_com2=False):
    """-> (status, ShiftedSystemProof buffers, the trace tensor the prover read)."""
    lib, ctx = D.lib(), D.context()
    L, W, P = mo["log_height"], mo["width"], mo["pre"]
    prog = CS.Program(wire)
    work = _dev(mo["matrix"] if matrix is None else matrix)
    src = work if committed is None else _dev(committed)
    handles = [_commit(src, L, W, 0, P)]
    if P < W and not drop_com2:
        handles.append(_commit(src, L, W, P, W - P))
    K = len(shifts) if n_shifts is None else n_shifts
    p = CS.ShiftedSystemProof(L, W, mo["degree"], P, mo["mask"], shifts[:K] if K <= len(shifts) else shifts)
    args = dict(sum=D.fe_bytes(mo["total"]), column_sum=D.fe_bytes(mo["column_sum"]), tr=tr.h,
                proof=ctypes.byref(p.c), matrix=D.ptr(work), shifts=_u32(shifts))
    if null:
        args[null] = None
    try:
        st = lib.mlh_system_prove_shifted(ctx, prog.h, handles[0],
                                          handles[1] if len(handles) > 1 else None,
                                          mo["mask"] if mask is None else mask, args["shifts"], K,
                                          args["matrix"], args["sum"], args["column_sum"], args["tr"],
                                          args["proof"])
    finally:
        for h in handles:
            lib.mlh_trace_commitment_destroy(h)
    p._sync()
    return st, p, work


def _verify(mo, wire, shifts, p, tr):
    prog = CS.Program(wire)
    return D.lib().mlh_system_verify_shifted(prog.h, mo["log_height"], mo["pre"], mo["mask"],
                                             _u32(shifts), len(shifts), D.fe_bytes(mo["total"]),
                                             D.fe_bytes(mo["column_sum"]), ctypes.byref(p.c), tr.h)


def _assert_pcs_equals_model(pcs, want):
    fp = pcs.fri_proof
    assert fp.batch_commitment == want["batch_commitment"]
    assert fp.commitments == want["commitments"]
    assert pcs.sumcheck_polynomials == [tuple(p) for p in want["polys"]]
    assert fp.last_elem == want["last_elem"]
    assert fp.last_random == want["last_random"]
    assert fp.query_indices == want["indices"]
    assert bytes(fp._q) == want["queries"]


@pytest.mark.parametrize("name", SR.GPU_NAMES)
def test_prove_matches_model_and_verifies(name):
    mo = SR.model(name)
    wire, shifts = SR.program(name)
    assert shifts == mo["shifts"]
    tr = _start(mo)
    entry = tr.clone()
    st, p, work = _prove(mo, wire, shifts, tr)
    assert st == 0, D.lib().mlh_last_error(D.context())
    c = p.c
    assert (c.log_height, c.width, c.degree, c.pre_random_columns, c.sum_column_mask, c.n_shifts) == \
        (mo["log_height"], mo["width"], mo["degree"], mo["pre"], mo["mask"], len(shifts))
    assert list(c.shift_columns) == shifts + [0] * (32 - len(shifts))
    assert _host(work) == mo["matrix"]  # dev_matrix is not modified
    assert p.sumcheck_polynomials == mo["pols"]
    assert p.output == mo["output"]
    assert p.shift_polynomials == mo["pols2"]
    assert p.output2 == mo["output2"]
    assert len(p.pcs) == len(mo["pcs"]) and len(p.pcs_shift) == len(mo["pcs_shift"])
    for got, want in zip(p.pcs + p.pcs_shift, mo["pcs"] + mo["pcs_shift"]):
        _assert_pcs_equals_model(got, want)
    assert tr.random() == mo["digest"]
    assert _verify(mo, wire, shifts, p, entry) == 0
    assert entry.random() == mo["digest"]


def test_no_shift_is_mlh_system_prove_phased():
    """K = 0: the phased proof's bytes and digest, and an unmodified trace."""
    name = "deg5_w7"
    mo = PR.model(name)
    L, W, P = mo["log_height"], mo["width"], mo["pre"]
    wire = S.program_wire(name)
    tr = _start(mo)
    st, p, work = _prove(mo, wire, [], tr)
    assert st == 0, D.lib().mlh_last_error(D.context())
    assert _host(work) == mo["matrix"]
    assert p.c.n_shifts == 0
    assert p.sumcheck_polynomials == mo["pols"] and p.output == mo["output"]
    for got, want in zip(p.pcs, mo["pcs"]):
        _assert_pcs_equals_model(got, want)
    assert tr.random() == mo["digest"]
    # and against the phased call itself, byte for byte
    lib, ctx = D.lib(), D.context()
    m = _dev(mo["matrix"])
    h1, h2 = _commit(m, L, W, 0, P), _commit(m, L, W, P, W - P)
    q = CS.PhasedSystemProof(L, W, mo["degree"], P, mo["mask"])
    t2 = _start(mo)
    try:
        assert lib.mlh_system_prove_phased(ctx, CS.Program(wire).h, h1, h2, mo["mask"], D.ptr(m),
                                           D.fe_bytes(mo["total"]), D.fe_bytes(mo["column_sum"]),
                                           t2.h, ctypes.byref(q.c)) == 0
    finally:
        lib.mlh_trace_commitment_destroy(h1)
        lib.mlh_trace_commitment_destroy(h2)
    q._sync()
    assert bytes(p._polys) == bytes(q._polys) and bytes(p._output) == bytes(q._output)
    for a, b in zip(p.pcs, q.pcs):
        assert bytes(a.c.fri.batch_commitment) == bytes(b.c.fri.batch_commitment)
        assert bytes(a.fri_proof._commit) == bytes(b.fri_proof._commit)
        assert bytes(a._polys) == bytes(b._polys)
        assert a.fri_proof.last_elem == b.fri_proof.last_elem
        assert a.fri_proof.last_random == b.fri_proof.last_random
        assert a.fri_proof.query_indices == b.fri_proof.query_indices
        assert bytes(a.fri_proof._q) == bytes(b.fri_proof._q)
    assert tr.random() == t2.random()
    assert _verify(mo, wire, [], p, _start(mo)) == 0


def test_openings_equal_standalone_batched_pcs():
    """Each of the four openings is byte-identical to mlh_batched_pcs_prove on
    its columns, run on a transcript that absorbed the same bytes."""
    name = "mixed5"
    mo = SR.model(name)
    wire, shifts = SR.program(name)
    L, W, P = mo["log_height"], mo["width"], mo["pre"]
    tr = _start(mo)
    st, p, _ = _prove(mo, wire, shifts, tr)
    assert st == 0
    m = _dev(mo["matrix"])
    cols = [CS.trace_columns(m, W, columns=(0, P)), CS.trace_columns(m, W, columns=(P, W - P))]

    def prefix_to(k):
        """The state before opening k: a transcript fed every byte up to it."""
        t = _start(mo)
        for root in p.commitments:
            t.absorb(root)
        t.absorb(F.to_bytes(mo["column_sum"]))
        t.absorb(mo["coeff_bytes"])
        assert t.random() == mo["after_sumcheck"]
        if k >= 2:  # the shift reduction's bytes, between the sumcheck and the openings
            t.absorb(b"".join(F.to_bytes(v) for v in p.output))
            t.absorb(mo["shift_bytes"])
            assert t.random() == mo["after_shift"]
        return t

    # the shift reduction absorbs before the first pair of openings too
    t2 = prefix_to(2)
    points = [(mo["rs"], p.output[:W]), (mo["rs2"], p.output2)]
    got = [p.pcs[0], p.pcs[1], p.pcs_shift[0], p.pcs_shift[1]]
    for k in range(4):
        at, vals = points[k // 2]
        rng = (0, P) if k % 2 == 0 else (P, W)
        alone = BatchedPCSProof.prove(at, vals[rng[0]:rng[1]], cols[k % 2], t2)
        g = got[k]
        assert bytes(alone.fri_proof.c.batch_commitment) == bytes(g.c.fri.batch_commitment)
        assert bytes(alone.fri_proof._commit) == bytes(g.fri_proof._commit)
        assert bytes(alone._polys) == bytes(g._polys)
        assert alone.fri_proof.last_elem == g.fri_proof.last_elem
        assert alone.fri_proof.last_random == g.fri_proof.last_random
        assert alone.fri_proof.query_indices == g.fri_proof.query_indices
        assert bytes(alone.fri_proof._q) == bytes(g.fri_proof._q)
    assert t2.random() == tr.random() == mo["digest"]


@pytest.mark.parametrize("name", ["fib_broken_mid", "fib_broken_wrap"])
def test_wrong_trace_proves_but_does_not_verify(name):
    mo = SR.model(name)
    wire, shifts = SR.program(name)
    tr = _start(mo)
    entry = tr.clone()
    st, p, _ = _prove(mo, wire, shifts, tr)
    assert st == 0
    assert p.output == mo["output"] and p.output2 == mo["output2"]
    assert _verify(mo, wire, shifts, p, entry) == VERIFY
    assert entry.random() == mo["entry"]


def test_trace_changed_after_the_commitment_does_not_verify():
    """The prover reads a trace other than the committed one: it cannot tell
    and returns MLH_OK; the verifier rejects."""
    name = "fib4"
    mo = SR.model(name)
    wire, shifts = SR.program(name)
    changed = list(mo["matrix"])
    changed[0] = (changed[0] + 1) % M
    tr = _start(mo)
    entry = tr.clone()
    st, p, _ = _prove(mo, wire, shifts, tr, matrix=changed, committed=mo["matrix"])
    assert st == 0
    assert _verify(mo, wire, shifts, p, entry) == VERIFY
    assert entry.random() == mo["entry"]


@pytest.mark.parametrize("what", ["duplicate_column", "column_at_W", "K_too_small", "K_too_large",
                                  "mask_bit_at_W", "null_shifts", "null_proof", "null_sum",
                                  "null_column_sum", "null_matrix", "com2_missing",
                                  "null_shift_polys", "null_output2"])
def test_prove_argument_errors_leave_transcript_unchanged(what):
    name = "mixed5"  # W = 4, P = 2, K = 1
    mo = SR.model(name)
    wire, shifts = SR.program(name)
    tr = _start(mo)
    kw = {"duplicate_column": dict(shifts=[2, 2], wire=SR.program("fib4")[0]),
          "column_at_W": dict(shifts=[4]),
          "K_too_small": dict(n_shifts=0),
          "K_too_large": dict(shifts=[2, 1]),
          "mask_bit_at_W": dict(mask=mo["mask"] | (1 << mo["width"])),
          "null_shifts": dict(null="shifts"), "null_proof": dict(null="proof"),
          "null_sum": dict(null="sum"), "null_column_sum": dict(null="column_sum"),
          "null_matrix": dict(null="matrix"), "com2_missing": dict(drop_com2=True),
          "null_shift_polys": {}, "null_output2": {}}[what]
    w = kw.pop("wire", wire)
    s = kw.pop("shifts", shifts)
    if what in ("null_shift_polys", "null_output2"):
        lib, ctx = D.lib(), D.context()
        work = _dev(mo["matrix"])
        h1, h2 = _commit(work, 5, 4, 0, 2), _commit(work, 5, 4, 2, 2)
        p = CS.ShiftedSystemProof(5, 4, mo["degree"], 2, mo["mask"], shifts)
        setattr(p.c, what[5:], None)
        try:
            st = lib.mlh_system_prove_shifted(ctx, CS.Program(wire).h, h1, h2, mo["mask"], _u32(shifts),
                                              1, D.ptr(work), D.fe_bytes(mo["total"]),
                                              D.fe_bytes(mo["column_sum"]), tr.h, ctypes.byref(p.c))
        finally:
            lib.mlh_trace_commitment_destroy(h1)
            lib.mlh_trace_commitment_destroy(h2)
    else:
        st, _, work = _prove(mo, w, s, tr, **kw)
    assert st == INVALID
    assert tr.random() == mo["entry"]
    assert _host(work) == mo["matrix"]


def test_width_limit_is_32_columns():
    """W + K = 33 cannot be expressed: a 32-wide program over a 17-wide trace
    with 16 shifts does not add up."""
    mo = SR.model("wide9")
    wire, shifts = SR.program("wide9")
    assert CS.Program(wire).width == 32
    tr = _start(mo)
    lib, ctx = D.lib(), D.context()
    m = D.to_device(D.random_limbs(17 << 9, 5))
    h = _commit(m, 9, 17, 0, 17)
    p = CS.ShiftedSystemProof(9, 17, 2, 17, 0, shifts)
    try:
        st = lib.mlh_system_prove_shifted(ctx, CS.Program(wire).h, h, None, 0, _u32(shifts), 16,
                                          D.ptr(m), D.fe_bytes(0), D.fe_bytes(0), tr.h,
                                          ctypes.byref(p.c))
    finally:
        lib.mlh_trace_commitment_destroy(h)
    assert st == INVALID
    assert tr.random() == mo["entry"]


# ---- Python mirror -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fib4", "mixed5"])
def test_python_mirror_round_trip(name):
    mo = SR.model(name)
    W = mo["width"]
    cset = CS.ConstraintSet(SR.exprs(name), mo["degree"])
    layout = CS.WitnessLayout(columns=W, randoms=mo["randoms"], pre_random_columns=mo["pre"],
                              sum_columns=mo["sum_columns"])
    trace = CS.Trace(_dev(mo["matrix"]), W)
    ext = trace.extend_next(mo["shifts"])
    assert ext.width() == W + len(mo["shifts"]) and _host(ext.matrix()) == mo["extension"]
    tr = _start(mo)
    vt = tr.clone()
    prover = CS.System.phased_prover(tr, cset, layout, trace)
    assert prover.shift_columns == mo["shifts"]
    assert prover.randoms == mo["trace_randoms"]
    proof = prover.prove(tr, mo["total"], mo["column_sum"])
    assert isinstance(proof, CS.ShiftedSystemProof)
    assert _host(trace.matrix()) == mo["matrix"]
    assert tr.random() == mo["digest"]
    assert proof.sumcheck_polynomials == mo["pols"] and proof.output == mo["output"]
    assert proof.shift_polynomials == mo["pols2"] and proof.output2 == mo["output2"]
    assert proof.verify(vt, cset, layout, mo["total"], mo["column_sum"])
    assert vt.random() == mo["digest"]
    bad = _start(mo)
    assert not proof.verify(bad, cset, layout, (mo["total"] + 1) % M, mo["column_sum"])
    assert bad.random() == mo["entry"]
