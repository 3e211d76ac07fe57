"""Public columns on the GPU: the strip written by mlh_trace_fill_public against
numpy, and the system proof with public columns (mlh_system_prove_public,
multilinear_amd's mirror) against the plain-Python model
tests/public_reference.py.  Every comparison is bit-exact."""
import ctypes

import numpy as np
import pytest

import public_reference as PUB
import shifted_reference as SR
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
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


# ---- mlh_trace_fill_public ----------------------------------------------------------

def _limbs(v):
    return np.frombuffer(int(v).to_bytes(16, "little"), dtype=np.uint32)


def np_strip(descs, H):
    """The H x F strip as (H, F, 4) uint32 limbs."""
    out = np.zeros((H, len(descs), 4), dtype=np.uint32)
    rows = np.arange(H, dtype=np.uint64)
    for j, d in enumerate(descs):
        if d[0] == "const":
            out[:, j] = _limbs(d[1])
        elif d[0] == "first":
            out[0, j, 0] = 1
        elif d[0] == "last":
            out[H - 1, j, 0] = 1
        elif d[0] == "row":
            out[:, j, 0] = (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            out[:, j, 1] = (rows >> np.uint64(32)).astype(np.uint32)
        elif d[0] == "periodic":
            table = np.stack([_limbs(v) for v in d[1]])
            out[:, j] = table[(rows % np.uint64(len(d[1]))).astype(np.int64)]
        else:
            for r, v in d[1].items():
                out[r, j] = _limbs(v)
    return out


def _info(log_height, width, n_public):
    return CS.public_fill_launch_info(log_height, width, n_public)


def _edge_rows(log_height, width, n_public):
    """Rows 0, H - 1, the last row of a tile and the first of the next."""
    H = 1 << log_height
    rows, _ = _info(log_height, width, n_public)
    return sorted(r for r in {0, H - 1, rows - 1, rows, H - rows - 1, H - rows} if 0 <= r < H)


def _values(seed, n):
    return [int.from_bytes(bytes(x), "little") for x in
            np.ascontiguousarray(D.random_limbs(n, seed)).view(np.uint8).reshape(n, 16)]


def _check_fill(log_height, width, descs, seed):
    H, Fn = 1 << log_height, len(descs)
    src = np.ascontiguousarray(D.random_limbs(H * width, seed)).reshape(H, width, 4)
    want = src.copy()
    want[:, width - Fn:] = np_strip(descs, H)
    m = D.to_device(src.reshape(H * width, 4))
    spec = PUB.builder(descs)
    D.check(D.lib().mlh_trace_fill_public(D.context(), spec.h, D.ptr(m), log_height, width),
            D.context())
    got = D.from_device(m).reshape(H, width, 4)
    assert np.array_equal(got[:, :width - Fn], src[:, :width - Fn])  # byte-identical below the strip
    assert np.array_equal(got, want)
    return got


def _sparse(log_height, width, n_public, vals):
    rows = _edge_rows(log_height, width, n_public)
    return ("sparse", {r: vals[i] for i, r in enumerate(rows)})


def _case(log_height, width, n_public):
    H = 1 << log_height
    v = _values(300 + log_height, 40)
    sp = _sparse(log_height, width, n_public, v)
    if (log_height, width, n_public) == (0, 1, 1):
        return [sp]
    if (log_height, width, n_public) == (1, 2, 1):
        return [("last",)]
    if (log_height, width, n_public) == (16, 2, 1):
        return [("periodic", _values(316, H))]  # k = 16 = L
    pool = [("first",), sp, ("periodic", v[8:12]), ("const", v[12]), ("row",), ("last",),
            ("periodic", v[13:14]), ("sparse", {H // 2: v[14]}), ("periodic", v[16:24]),
            ("const", 0), ("last",), ("row",), ("first",), ("const", M - 1), sp,
            ("periodic", v[24:26])]
    return pool[:n_public]


@pytest.mark.parametrize("log_height,width,n_public", [(0, 1, 1), (1, 2, 1), (5, 7, 3), (9, 32, 16),
                                                       (12, 17, 5), (16, 2, 1)])
def test_fill_public_matches_numpy(log_height, width, n_public):
    descs = _case(log_height, width, n_public)
    assert len(descs) == n_public
    got = _check_fill(log_height, width, descs, 50 + log_height)
    if log_height <= 9:  # numpy's strip against the model's plain indexing
        H = 1 << log_height
        strip = got[:, width - n_public:].reshape(H * n_public, 4)
        assert D.limbs_to_ints(strip) == PUB.strip(descs, H)


def test_fill_public_one_row_is_first_and_last():
    got = _check_fill(0, 6, [("first",), ("last",), ("row",), ("periodic", [5]), ("const", 7)], 3)
    assert [int(x) for x in got[0, 1:, 0]] == [1, 1, 0, 5, 7]


def test_fill_public_sparse_limit():
    """m = 4096 entries in one column, beside a second sparse column."""
    L, width = 13, 3
    v = _values(41, 4096)
    rows = [2 * i + (i * 37 % 2) for i in range(4096)]  # strictly increasing, in every tile
    assert rows == sorted(set(rows)) and rows[-1] < (1 << L)
    _check_fill(L, width, [("sparse", dict(zip(rows, v))), _sparse(L, width, 2, v)], 42)


def test_fill_public_block_loops_over_tiles():
    """2^18 x 16 with F = 16: 2^22 strip elements, 2048 tiles of 2048 elements
    on 1024 blocks -- every block visits two tiles."""
    L, width, Fn = 18, 16, 16
    rows, blocks = _info(L, width, Fn)
    tiles = (1 << L) // rows
    print("fill_public 2^%d x %d, F = %d: %d tiles of %d rows on %d blocks" % (L, width, Fn, tiles,
                                                                               rows, blocks))
    assert (rows, blocks, tiles) == (128, 1024, 2048)
    rows_lower, blocks_lower = _info(L - 1, width, Fn)
    assert (1 << (L - 1)) // rows_lower == blocks_lower  # one tile per block below
    H = 1 << L
    v = _values(43, 64)
    sp = ("sparse", {r: v[i] for i, r in enumerate(
        sorted({0, H - 1, rows - 1, rows, blocks * rows - 1, blocks * rows, H - rows}))})
    descs = [("first",), sp, ("periodic", v[8:12]), ("const", v[12]), ("row",), ("last",),
             ("periodic", v[13:14]), ("sparse", {H // 2: v[14]}), ("periodic", v[16:48]),
             ("const", 0), ("last",), ("row",), ("first",), ("const", M - 1), sp,
             ("periodic", v[48:50])]
    _check_fill(L, width, descs, 44)


def test_fill_public_argument_errors():
    lib, ctx = D.lib(), D.context()
    src = D.random_limbs(4 * 3, 9)
    m = D.to_device(src)
    spec = PUB.builder([("first",), ("row",)])
    f = lib.mlh_trace_fill_public
    assert f(None, spec.h, D.ptr(m), 2, 3) == INVALID
    assert f(ctx, None, D.ptr(m), 2, 3) == INVALID
    assert f(ctx, spec.h, None, 2, 3) == INVALID
    assert f(ctx, spec.h, D.ptr(m), 2, 1) == INVALID  # F > width
    assert f(ctx, spec.h, D.ptr(m), 2, 0) == INVALID
    assert f(ctx, spec.h, D.ptr(m), 2, 33) == INVALID
    assert f(ctx, spec.h, D.ptr(m), 33, 3) == INVALID
    assert f(ctx, PUB.builder([("periodic", list(range(8)))]).h, D.ptr(m), 2, 3) == INVALID  # k > L
    assert f(ctx, PUB.builder([("sparse", {4: 1})]).h, D.ptr(m), 2, 3) == INVALID  # row 4 of 4
    assert np.array_equal(D.from_device(m), src)  # the matrix is untouched
    rows, blocks = ctypes.c_uint32(), ctypes.c_uint32()
    g = lib.mlh_trace_fill_public_launch_info
    assert g(3, 4, 2, ctypes.byref(rows), ctypes.byref(blocks)) == 0
    assert (rows.value, blocks.value) == (8, 1)
    assert g(3, 33, 2, ctypes.byref(rows), ctypes.byref(blocks)) == INVALID
    assert g(3, 4, 5, ctypes.byref(rows), ctypes.byref(blocks)) == INVALID
    assert g(3, 20, 17, ctypes.byref(rows), ctypes.byref(blocks)) == INVALID
    assert g(3, 4, 0, ctypes.byref(rows), ctypes.byref(blocks)) == INVALID
    assert g(3, 4, 2, None, ctypes.byref(blocks)) == INVALID
    assert f(ctx, spec.h, D.ptr(m), 2, 3) == 0


# ---- mlh_system_prove_public --------------------------------------------------------

def _commit(m, L, W, col0, ncols):
    h = ctypes.c_void_p()
    D.check(D.lib().mlh_trace_commit_range(D.context(), D.ptr(m), L, W, col0, ncols, ctypes.byref(h)),
            D.context())
    return h


def _prove(mo, wire, shifts, tr, spec, matrix=None, ranges=None, n_public=None):
    """-> (status, ShiftedSystemProof buffers, the trace tensor the prover read).
    ranges: the (col0, ncols) of the commitments, by default [0, P) and [P, W - F)."""
    lib, ctx = D.lib(), D.context()
    L, W, P, C = mo["log_height"], mo["width"], mo["pre"], mo["committed"]
    prog = CS.Program(wire)
    work = _dev(mo["matrix"] if matrix is None else matrix)
    if ranges is None:
        ranges = [(0, P)] + ([(P, C - P)] if P < C else [])
    handles = [_commit(work, L, W, c0, n) for c0, n in ranges]
    p = CS.ShiftedSystemProof(L, W, mo["degree"], P, mo["mask"], shifts,
                              mo["n_public"] if n_public is None else n_public)
    try:
        st = lib.mlh_system_prove_public(ctx, prog.h, handles[0],
                                         handles[1] if len(handles) > 1 else None, mo["mask"],
                                         _u32(shifts), len(shifts), spec.h if spec else None,
                                         D.ptr(work), D.fe_bytes(mo["total"]),
                                         D.fe_bytes(mo["column_sum"]), tr.h, ctypes.byref(p.c))
    finally:
        for h in handles:
            lib.mlh_trace_commitment_destroy(h)
    p._sync()
    return st, p, work


def _verify(mo, wire, shifts, p, tr, spec):
    prog = CS.Program(wire)
    return D.lib().mlh_system_verify_public(prog.h, mo["log_height"], mo["pre"], mo["mask"],
                                            _u32(shifts), len(shifts), spec.h if spec else None,
                                            D.fe_bytes(mo["total"]), D.fe_bytes(mo["column_sum"]),
                                            ctypes.byref(p.c), tr.h)


def _assert_pcs_equals_model(pcs, want):
    fp = pcs.fri_proof
    assert fp.batch_commitment == want["batch_commitment"]
    assert fp.commitments == want["commitments"]
    assert pcs.sumcheck_polynomials == [tuple(p) for p in want["polys"]]
    assert fp.last_elem == want["last_elem"]
    assert fp.last_random == want["last_random"]
    assert fp.query_indices == want["indices"]
    assert bytes(fp._q) == want["queries"]


def _proof_bytes(p):
    out = [bytes(p._polys), bytes(p._output), bytes(p._shift_polys), bytes(p._output2)]
    for a in p.pcs + p.pcs_shift:
        fp = a.fri_proof
        out += [bytes(a.c.fri.batch_commitment), bytes(fp._commit), bytes(a._polys),
                F.to_bytes(fp.last_elem), fp.last_random, bytes(fp._q)]
    return out


@pytest.mark.parametrize("name", PUB.GPU_NAMES)
def test_prove_matches_model_and_verifies(name):
    mo = PUB.model(name)
    wire, shifts = PUB.program(name)
    assert shifts == mo["shifts"]
    spec = PUB.builder(mo["descs"])
    assert spec.wire == mo["wire"]
    L, W, C = mo["log_height"], mo["width"], mo["committed"]
    # the strip the kernel writes is the model's
    t = CS.Trace(_dev([0 if j >= C else mo["matrix"][i * W + j] for i in range(1 << L)
                       for j in range(W)]), W)
    t.fill_public(spec)
    assert _host(t.matrix()) == mo["matrix"]
    tr = _start(mo)
    entry = tr.clone()
    st, p, work = _prove(mo, wire, shifts, tr, spec)
    assert st == 0, D.lib().mlh_last_error(D.context())
    c = p.c
    assert (c.log_height, c.width, c.degree, c.pre_random_columns, c.sum_column_mask, c.n_shifts) == \
        (L, W, mo["degree"], mo["pre"], mo["mask"], len(shifts))
    assert _host(work) == mo["matrix"]  # dev_matrix is not modified
    assert p.sumcheck_polynomials == mo["pols"]
    assert p.output == mo["output"]
    assert p.shift_polynomials == mo["pols2"]
    assert p.output2 == mo["output2"]
    assert len(p.pcs) == len(mo["pcs"]) and len(p.pcs_shift) == len(mo["pcs_shift"])
    assert [q.c.fri.num_codes for q in p.pcs] == [mo["pre"]] + [C - mo["pre"]] * (len(p.pcs) - 1)
    for got, want in zip(p.pcs + p.pcs_shift, mo["pcs"] + mo["pcs_shift"]):
        _assert_pcs_equals_model(got, want)
    assert tr.random() == mo["digest"]
    assert _verify(mo, wire, shifts, p, entry, spec) == 0
    assert entry.random() == mo["digest"]


@pytest.mark.parametrize("name", ["fib4", "mixed5"])
def test_no_spec_is_mlh_system_prove_shifted(name):
    """spec = NULL: the shifted proof's bytes and final transcript state."""
    mo = dict(SR.model(name))
    mo.update(committed=mo["width"], n_public=0)
    wire, shifts = SR.program(name)
    tr = _start(mo)
    st, p, _ = _prove(mo, wire, shifts, tr, None)
    assert st == 0, D.lib().mlh_last_error(D.context())
    lib, ctx = D.lib(), D.context()
    L, W, P = mo["log_height"], mo["width"], mo["pre"]
    m = _dev(mo["matrix"])
    handles = [_commit(m, L, W, 0, P)] + ([_commit(m, L, W, P, W - P)] if P < W else [])
    q = CS.ShiftedSystemProof(L, W, mo["degree"], P, mo["mask"], shifts)
    t2 = _start(mo)
    try:
        assert lib.mlh_system_prove_shifted(ctx, CS.Program(wire).h, handles[0],
                                            handles[1] if len(handles) > 1 else None, mo["mask"],
                                            _u32(shifts), len(shifts), D.ptr(m),
                                            D.fe_bytes(mo["total"]), D.fe_bytes(mo["column_sum"]),
                                            t2.h, ctypes.byref(q.c)) == 0
    finally:
        for h in handles:
            lib.mlh_trace_commitment_destroy(h)
    q._sync()
    assert _proof_bytes(p) == _proof_bytes(q)
    assert tr.random() == t2.random() == mo["digest"]
    assert _verify(mo, wire, shifts, p, _start(mo), None) == 0


def _random_ab(H, seed):
    """Random a, b for H rows, interleaved."""
    return _values(seed, 2 * H)


def test_the_gap_a_committed_selector_proves_anything():
    """What public columns close: with the wrap gate `last` a committed column,
    a prover who commits last = 1 on every row turns the Fibonacci constraints
    into 0 = 0, and the shifted proof of random a, b verifies with total 0."""
    L, H = 4, 16
    ab = _random_ab(H, 61)
    matrix = [x for i in range(H) for x in (ab[2 * i], ab[2 * i + 1], 1)]
    wire, shifts = SR.program("fib4")
    mo = dict(seed=b"gap", log_height=L, width=3, pre=3, committed=3, n_public=0, degree=2, mask=0,
              matrix=matrix, total=0, column_sum=0)
    tr = _start(mo)
    entry = tr.clone()
    st, p, _ = _prove(mo, wire, shifts, tr, None)
    assert st == 0
    assert D.lib().mlh_system_verify_shifted(CS.Program(wire).h, L, 3, 0, _u32(shifts), 2,
                                             D.fe_bytes(0), D.fe_bytes(0), ctypes.byref(p.c),
                                             entry.h) == 0


@pytest.mark.parametrize("strip", ["ones", "gates_open"])
def test_the_closure_a_forged_strip_does_not_verify(strip):
    """The same random a, b under the statement with public columns.  The
    prover fills the strip, then overwrites it -- with ones, or with last = 1,
    first = 0, io = b, which makes every constraint vanish so that both sumchecks are
    consistent with total 0: mlh_system_prove_public cannot tell and returns
    MLH_OK, the verifier's own evaluation of the spec rejects."""
    base = PUB.model("pfib4")
    L, H, W = 4, 16, 5
    ab = _random_ab(H, 61)
    # gates_open: (first, last, io) = (0, 1, b) on every row
    matrix = [x for i in range(H) for x in [ab[2 * i], ab[2 * i + 1]] +
              ([1, 1, 1] if strip == "ones" else [0, 1, ab[2 * i + 1]])]
    spec = PUB.builder(base["descs"])
    wire, shifts = PUB.program("pfib4")
    mo = dict(base, seed=b"gap", matrix=matrix)
    t = CS.Trace(_dev(matrix), W)
    t.fill_public(spec)
    assert _host(t.matrix())[2:5] == [1, 0, 1]  # the fill wrote first, last, io on row 0
    tr = _start(mo)
    entry = tr.clone()
    before = entry.random()
    st, p, _ = _prove(mo, wire, shifts, tr, spec)  # the strip overwritten after the fill
    assert st == 0
    assert _verify(mo, wire, shifts, p, entry, spec) == VERIFY
    assert entry.random() == before


def test_wrong_start_proves_but_does_not_verify():
    """A trace started from a != io[0]."""
    mo = PUB.model("pfib4_wrong_start")
    wire, shifts = PUB.program("pfib4")
    spec = PUB.builder(mo["descs"])
    tr = _start(mo)
    entry = tr.clone()
    st, p, _ = _prove(mo, wire, shifts, tr, spec)
    assert st == 0
    assert p.output == mo["output"] and p.output2 == mo["output2"]
    assert _verify(mo, wire, shifts, p, entry, spec) == VERIFY
    assert entry.random() == mo["entry"]


@pytest.mark.parametrize("what", ["widths_do_not_add_up", "as_many_public_as_columns", "spec_too_tall",
                                  "period_too_long", "com2_although_all_pre_random",
                                  "spec_missing"])
def test_prove_argument_errors_leave_transcript_unchanged(what):
    name = "pfib4"  # W = 5, P = 2, F = 3, K = 2
    mo = PUB.model(name)
    wire, shifts = PUB.program(name)
    ds = mo["descs"]
    spec, kw = PUB.builder(ds), {}
    if what == "widths_do_not_add_up":
        kw = dict(ranges=[(0, 3)])
    elif what == "as_many_public_as_columns":
        spec, kw = PUB.builder(ds + [("row",), ("first",)]), dict(n_public=3)
    elif what == "spec_too_tall":
        spec = PUB.builder([ds[0], ds[1], ("sparse", {0: 1, 16: 2})])
    elif what == "period_too_long":
        spec = PUB.builder([ds[0], ds[1], ("periodic", list(range(32)))])
    elif what == "com2_although_all_pre_random":
        kw = dict(ranges=[(0, 2), (2, 1)])
    else:
        spec = None  # F = 0: 2 committed columns of 5
    tr = _start(mo)
    st, _, work = _prove(mo, wire, shifts, tr, spec, **kw)
    assert st == INVALID
    assert tr.random() == mo["entry"]
    assert _host(work) == mo["matrix"]


# ---- Python mirror -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pfib4", "pmixed5"])
def test_python_mirror_round_trip(name):
    mo = PUB.model(name)
    W, C, H = mo["width"], mo["committed"], 1 << mo["log_height"]
    cset = CS.ConstraintSet(PUB.exprs(name), mo["degree"])
    layout = CS.WitnessLayout(columns=W, randoms=mo["randoms"], pre_random_columns=mo["pre"],
                              sum_columns=mo["sum_columns"], public_columns=PUB.builder(mo["descs"]))
    assert layout.n_public == W - C
    # the strip arrives unwritten: phased_prover fills it
    trace = CS.Trace(_dev([7 if j >= C else mo["matrix"][i * W + j] for i in range(H)
                           for j in range(W)]), W)
    tr = _start(mo)
    vt = tr.clone()
    prover = CS.System.phased_prover(tr, cset, layout, trace)
    assert _host(trace.matrix()) == mo["matrix"]
    assert prover.shift_columns == mo["shifts"]
    assert prover.randoms == mo["trace_randoms"]
    assert tr.random() == mo["entry"]
    proof = prover.prove(tr, mo["total"], mo["column_sum"])
    assert isinstance(proof, CS.ShiftedSystemProof) and proof.n_public == W - C
    assert _host(trace.matrix()) == mo["matrix"]
    assert tr.random() == mo["digest"]
    assert proof.sumcheck_polynomials == mo["pols"] and proof.output == mo["output"]
    assert proof.shift_polynomials == mo["pols2"] and proof.output2 == mo["output2"]
    assert proof.commitments == [q["batch_commitment"] for q in mo["pcs"]]
    assert proof.output[C:W] == layout.public_columns.evaluate(mo["rs"])
    # the verifier's own spec, built apart from the prover's
    assert proof.verify(vt, cset, layout, mo["total"], mo["column_sum"], public=PUB.builder(mo["descs"]))
    assert vt.random() == mo["digest"]
    assert proof.verify(_start(mo), cset, layout, mo["total"], mo["column_sum"])
    bad = _start(mo)
    other = PUB.builder(mo["descs"][:-1] + [("const", 1)])
    assert not proof.verify(bad, cset, layout, mo["total"], mo["column_sum"], public=other)
    assert bad.random() == mo["entry"]
    assert not proof.verify(bad, cset, layout, (mo["total"] + 1) % M, mo["column_sum"])
    assert bad.random() == mo["entry"]
