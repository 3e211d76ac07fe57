"""mlh_trace_scan on the GPU: running sums and running products down columns of
a device trace against the plain-Python model tests/scan_reference.py, under
the default launch and under the shapes of mlh_trace_scan_shaped where the
seams are (the carry between a block's tiles, uneven and empty block ranges,
many blocks), up to a permutation argument proved through PhasedProver with
the grand product scanned on the device.  Every comparison is bit-exact."""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

import scan_reference as SR
import stream_harness as H
import test_stream_contract_gpu as TSC
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.transcript import Transcript

pytestmark = pytest.mark.gpu

M = SR.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]

# (threads, rows per thread, max blocks) of mlh_trace_scan_shaped
SHAPES = [(64, 1, 1),       # many tiles in one block: the carry between tiles
          (64, 2, 3),       # uneven ranges and, at small heights, blocks with an empty range
          (128, 4, 2),
          (256, 16, 1024)]
MANY_BLOCKS = (64, 1, 1024)  # at 2^12 rows: 64 blocks of one tile


# ---- helpers -----------------------------------------------------------------------------

def _u8(vals):
    vals = list(vals)
    return (ctypes.c_uint8 * max(len(vals), 1))(*vals)


def _scan(mat, W, scans, shape=None, totals=True):
    """mat: (H * W, 4) uint32 limbs on the host.  -> (the matrix after the call
    as such an array, the totals or None).  shape None: mlh_trace_scan."""
    L = (mat.shape[0] // W).bit_length() - 1
    m = D.to_device(mat)
    if shape is None:
        tot = CS.Trace(m, W).scan(scans, totals=totals)
    else:
        ops, src, dst, inits = CS._scan_arrays(scans, W)
        n = len(ops)
        out = (ctypes.c_uint8 * (16 * n))() if totals else None
        ctx = D.context()
        st = D.lib().mlh_trace_scan_shaped(ctx, D.ptr(m), L, W, n, _u8(ops), _u8(src), _u8(dst),
                                           CS._elems(inits), out, *shape)
        assert st == 0, D.lib().mlh_last_error(ctx)
        tot = CS._split(out, n) if totals else None
    return D.from_device(m), tot


def _model(mat, W, scans):
    """The model on the columns the scans touch (the others stay as they are):
    -> (the expected matrix as limbs, the totals)."""
    a = mat.reshape(-1, W, 4)
    used = sorted({c for _, s, d, _ in scans for c in (s, d)})
    at = {c: k for k, c in enumerate(used)}
    small = D.limbs_to_ints(np.ascontiguousarray(a[:, used, :]))
    out, totals = SR.scan_matrix(small, len(used), [(op, at[s], at[d], i) for op, s, d, i in scans])
    want = a.copy()
    want[:, used, :] = D.ints_to_limbs(out).reshape(-1, len(used), 4)
    return want.reshape(-1, 4), totals


def _check(mat, W, scans, shapes):
    """The model's bytes and totals under every shape of ``shapes`` (None: the
    default launch)."""
    want, totals = _model(mat, W, scans)
    for shape in shapes:
        got, tot = _scan(mat, W, scans, shape)
        assert np.array_equal(got, want), shape
        assert tot == totals, shape
    return want, totals


def _tile_log(shape):
    return (shape[0] * shape[1]).bit_length() - 1


def _default_heights():
    """Around one tile of the default rule, from mlh_trace_scan_launch_info."""
    threads, rows, _ = CS.trace_scan_launch_info(0, 1, 1)
    top = (threads * rows).bit_length() - 1
    return sorted({min(L, 14) for L in (0, 1, 6, top - 1, top, top + 1, top + 3)})


def _inits(seed):
    r = random.Random(seed)
    return r.randrange(M), r.randrange(1, M)


# ---- the default launch ----------------------------------------------------------------------

@pytest.mark.parametrize("log_height", _default_heights())
@pytest.mark.parametrize("width", [1, 3, 8, 32])
def test_default_launch_matches_model(width, log_height):
    mat = D.random_limbs(width << log_height, 1000 * width + log_height)
    i_add, i_mul = _inits("d %d %d" % (width, log_height))
    if width == 1:  # one column: the two scans in place, one call each
        _check(mat, 1, [("add", 0, 0, i_add)], [None])
        _check(mat, 1, [("mul", 0, 0, i_mul)], [None])
    else:
        _check(mat, width, [("add", 0, 1, i_add), ("mul", width - 1, width - 1, i_mul)], [None])


def test_default_launch_reaches_several_blocks():
    """The heights above cover one block (the apply launch alone) and several
    (all three launches)."""
    blocks = [CS.trace_scan_launch_info(L, 8, 2)[2] for L in _default_heights()]
    assert blocks[0] == 1 and blocks[-1] > 2


# ---- explicit shapes: the seams ------------------------------------------------------------------

SEAMS = [(shape, L) for shape in SHAPES
         for L in range(_tile_log(shape) - 1, _tile_log(shape) + 4)] + [(MANY_BLOCKS, 12)]


@pytest.mark.parametrize("shape,log_height", SEAMS)
def test_shaped_launch_matches_model_and_default(shape, log_height):
    """From half a tile to 8 tiles: the shape and the default launch give the
    model's bytes."""
    W = 3
    mat = D.random_limbs(W << log_height, 77 + log_height)
    i_add, i_mul = _inits("s %r %d" % (shape, log_height))
    _check(mat, W, [("add", 2, 0, i_add), ("mul", 1, 1, i_mul)], [shape, None])


# ---- values that find bugs -------------------------------------------------------------------------

ZERO_SHAPE = (64, 2, 3)  # tiles of 128 rows, 4 tiles on 3 blocks: 2 + 2 + 0


@functools.lru_cache(maxsize=None)
def _zero_base():
    return D.random_limbs(2 << 9, 4242)


@pytest.mark.parametrize("where", ["tile_end", "tile_start", "row0", "last_row", "absent"])
def test_product_scan_with_a_zero(where):
    """Everything after a zero is zero; the total is zero unless the zero is
    absent."""
    W, Hh, T = 2, 1 << 9, ZERO_SHAPE[0] * ZERO_SHAPE[1]
    row = {"tile_end": T - 1, "tile_start": T, "row0": 0, "last_row": Hh - 1, "absent": None}[where]
    mat = _zero_base().copy()
    if row is not None:
        mat[row * W] = 0
    want, totals = _check(mat, W, [("mul", 0, 1, 1)], [ZERO_SHAPE, None, (64, 1, 1)])
    z = D.limbs_to_ints(np.ascontiguousarray(want.reshape(-1, W, 4)[:, 1, :]))
    if row is None:
        assert all(z) and totals[0] != 0
    else:
        assert all(z[:row + 1]) and not any(z[row + 1:]) and totals == [0]


@pytest.mark.parametrize("init", [0, 1, M - 1, 0x0123456789ABCDEF0123456789ABCDEF % M])
def test_edge_elements_and_inits(init):
    """Products of M - 1 and 1 (the running value flips between init and
    -init), and sums of elements >= M - 2^40, where every addition wraps."""
    W, L = 3, 11
    r = random.Random(99)
    rows = 1 << L
    vals = []
    for _ in range(rows):
        vals += [r.choice((M - 1, 1)), M - 1 - r.randrange(1 << 40), r.randrange(M)]
    mat = D.ints_to_limbs(vals)
    other = (init + (1 << 100)) % M  # far above rows * 2^40: no running sum comes near zero
    want, _ = _check(mat, W, [("mul", 0, 0, init), ("add", 1, 2, other)], [None, ZERO_SHAPE, (128, 4, 2)])
    z = D.limbs_to_ints(np.ascontiguousarray(want.reshape(-1, W, 4)[:, 0, :]))
    assert set(z) <= {init, (M - init) % M}
    s = D.limbs_to_ints(np.ascontiguousarray(want.reshape(-1, W, 4)[:, 2, :]))
    # z + t >= M at every row: the reduced sum is below z by M - t, at most 2^40
    assert (1 << 99) < other and all(0 < s[i] - s[i + 1] <= 1 << 40 for i in range(rows - 1))
    _check(mat, W, [("add", 1, 1, init)], [None, (64, 1, 1)])


# ---- eight scans at once ---------------------------------------------------------------------------

def _eight_scans_w9():
    r = random.Random(8)
    i = [r.randrange(M) for _ in range(8)]
    return [("mul", 0, 0, i[0]),   # in place
            ("add", 1, 2, i[1]),
            ("mul", 2, 3, i[2]),   # its source is the destination of the scan before
            ("add", 4, 4, i[3]),   # in place
            ("add", 5, 6, i[4]),   # two scans
            ("mul", 5, 7, i[5]),   # ... of one source
            ("add", 3, 1, i[6]),   # source: another scan's destination; destination: another's source
            ("mul", 8, 5, i[7])]   # overwrites the shared source; column 8 is read only


def test_eight_scans_snapshot_semantics():
    W, L = 9, 12
    mat = D.random_limbs(W << L, 909)
    scans = _eight_scans_w9()
    want, _ = _check(mat, W, scans, [None] + SHAPES + [MANY_BLOCKS])
    assert np.array_equal(want.reshape(-1, W, 4)[:, 8, :], mat.reshape(-1, W, 4)[:, 8, :])
    # the model really is the snapshot: scan 2 summed the old column 2, not scan 1's output
    old2 = D.limbs_to_ints(np.ascontiguousarray(mat.reshape(-1, W, 4)[:2, 2, :]))
    z3 = D.limbs_to_ints(np.ascontiguousarray(want.reshape(-1, W, 4)[:2, 3, :]))
    assert z3 == [scans[2][3], scans[2][3] * old2[0] % M]


def test_eight_of_32_columns_and_the_rest_untouched():
    W, L = 32, 11
    mat = D.random_limbs(W << L, 3232)
    r = random.Random(32)
    dst = [31, 0, 7, 8, 15, 16, 24, 25]
    src = [31, 1, 8, 7, 30, 30, 2, 16]
    scans = [("mul" if k % 2 else "add", src[k], dst[k], r.randrange(M)) for k in range(8)]
    want, _ = _model(mat, W, scans)
    for shape in (None, (64, 2, 3), (256, 16, 1024)):
        got, _ = _scan(mat, W, scans, shape)
        assert np.array_equal(got, want), shape
        keep = [c for c in range(W) if c not in dst]
        assert got.reshape(-1, W, 4)[:, keep, :].tobytes() == mat.reshape(-1, W, 4)[:, keep, :].tobytes()


@pytest.mark.parametrize("n_scans", [1, 2, 3, 4, 5, 8])
def test_every_scan_count_builds_the_same_columns(n_scans):
    """1 .. 8 scans (the kernels are built for up to 1, 2, 4 and 8): the first
    n of the eight, on several blocks."""
    W, L = 9, 11
    mat = D.random_limbs(W << L, 500 + n_scans)
    _check(mat, W, _eight_scans_w9()[:n_scans], [None, (64, 2, 3)])


# ---- totals_out ----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [None, (64, 1, 1), (64, 2, 3)])
def test_without_totals_the_matrix_is_the_same(shape):
    W, L = 4, 11
    mat = D.random_limbs(W << L, 31)
    scans = [("mul", 0, 1, 1), ("add", 2, 2, 5)]
    want, totals = _model(mat, W, scans)
    got, tot = _scan(mat, W, scans, shape, totals=True)
    assert tot == totals and np.array_equal(got, want)
    got, tot = _scan(mat, W, scans, shape, totals=False)
    assert tot is None and np.array_equal(got, want)


# ---- argument errors ---------------------------------------------------------------------------------

_OK = dict(log_height=6, width=4, n=2, ops=[0, 1], src=[0, 1], dst=[2, 3], inits=[5, 7],
           shape=(256, 4, 1024))
BAD = {
    "width 0": dict(width=0), "width 33": dict(width=33), "log_height 33": dict(log_height=33),
    "no scan": dict(n=0), "nine scans": dict(n=9, ops=[0] * 9, src=[0] * 9, dst=list(range(9)),
                                             inits=[1] * 9, width=16),
    "op 2": dict(ops=[0, 2]), "source at width": dict(src=[0, 4]),
    "destination at width": dict(dst=[2, 4]), "destination twice": dict(dst=[3, 3]),
    "init M": dict(inits=[5, M]), "init 2^128 - 1": dict(inits=[(1 << 128) - 1, 7]),
    "null matrix": dict(matrix=None), "null ops": dict(ops=None), "null sources": dict(src=None),
    "null destinations": dict(dst=None), "null inits": dict(inits=None),
    "threads 32": dict(shape=(32, 4, 8)), "threads 512": dict(shape=(512, 4, 8)),
    "threads 96": dict(shape=(96, 4, 8)), "rows 0": dict(shape=(64, 0, 8)),
    "rows 3": dict(shape=(64, 3, 8)), "rows 32": dict(shape=(64, 32, 8)),
    "no block": dict(shape=(64, 4, 0)), "1025 blocks": dict(shape=(64, 4, 1025)),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_errors_leave_the_matrix_alone(what):
    a = dict(_OK, **BAD[what])
    mat = D.random_limbs(16 << 6, 5)  # room for the widest case that could be taken as valid
    m = D.to_device(mat)
    lib, ctx = D.lib(), D.context()
    tot = (ctypes.c_uint8 * (16 * 9))()
    arr = lambda v: None if v is None else _u8(v)
    inits = None if a["inits"] is None else (ctypes.c_uint8 * (16 * len(a["inits"]))).from_buffer_copy(
        b"".join(int(v).to_bytes(16, "little") for v in a["inits"]))
    mp = D.ptr(m) if a.get("matrix", True) is not None else None
    args = (mp, a["log_height"], a["width"], a["n"], arr(a["ops"]), arr(a["src"]), arr(a["dst"]), inits)
    calls = [lambda t: lib.mlh_trace_scan_shaped(ctx, *args, t, *a["shape"])]
    if a["shape"] == _OK["shape"]:
        calls.append(lambda t: lib.mlh_trace_scan(ctx, *args, t))
    for call in calls:
        for t in (tot, None):
            assert call(t) == INVALID, what
            assert lib.mlh_last_error(ctx)
    torch.cuda.synchronize()
    assert np.array_equal(D.from_device(m), mat)
    assert lib.mlh_trace_scan(None, *args, tot) == INVALID


def test_mirror_rejects_before_the_library():
    t = CS.Trace(D.to_device(D.random_limbs(4 << 3, 1)), 4)
    before = D.from_device(t.matrix()).copy()
    for scans in ([("add", 0, 1, 0), ("mul", 2, 1, 1)], [("add", 0, 4, 0)], [("xor", 0, 1, 0)], []):
        with pytest.raises(ValueError):
            t.scan(scans)
    with pytest.raises(_lib.MlhError):
        t.scan([("add", 0, 1, M)])
    assert np.array_equal(D.from_device(t.matrix()), before)


# ---- the stream contract ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def S():
    return H.side_stream()


def test_scan_behind_pending_work(S):
    """totals_out NULL: the call does not wait; on a busy side stream with the
    matrix arriving late it gives the bytes of the default stream."""
    lib, L, W = D.lib(), 11, 5
    a = D.random_limbs(W << L, 321)
    scans = [("mul", 0, 0, 3), ("add", 1, 4, 9), ("add", 4, 2, 0)]
    want, _ = _check(a, W, scans, [None])  # the default stream
    ops, src, dst, inits = CS._scan_arrays(scans, W)

    def op(buf):  # in place
        TSC._call(lib.mlh_trace_scan, D.ptr(buf), L, W, 3, _u8(ops), _u8(src), _u8(dst),
                  CS._elems(inits), None)
        return buf

    TSC._both(TSC._enqueue(S, "trace_scan (11, 5)", [a], op), want)


def test_scan_totals_with_late_trace(S):
    """With totals_out the call synchronises: totals and matrix of the late
    trace, not of what stood in the buffer before."""
    L, W = 11, 5
    a = D.random_limbs(W << L, 322)
    scans = [("mul", 2, 3, 1), ("add", 0, 0, 7)]
    want, totals = _model(a, W, scans)

    def call(buf):
        tot = CS.Trace(buf, W).scan(scans)
        return tot, D.from_device(buf).tobytes()

    TSC._same(TSC._returns(S, "trace_scan totals (11, 5)", [a], call), (totals, want.tobytes()))


# ---- scratch poison ----------------------------------------------------------------------------------

def test_scratch_poison_does_not_reach_the_output():
    """The aggregates, offsets and totals come from the pool: under two
    different poison words, at shapes with several blocks (some of them with an
    empty range), the same bytes both times and the model's."""
    W, L = 9, 11
    mat = D.random_limbs(W << L, 606)
    scans = _eight_scans_w9()
    want, totals = _model(mat, W, scans)
    lib, ctx = D.lib(), D.context()
    results = []
    try:
        for word in (3, 0x01234567):
            for shape in (None, (64, 2, 3), MANY_BLOCKS):
                D.check(lib.mlh_set_scratch_poison(ctx, word), ctx)
                results.append(_scan(mat, W, scans, shape))
    finally:
        D.check(lib.mlh_set_scratch_poison(ctx, 0), ctx)
    for got, tot in results:
        assert np.array_equal(got, want) and tot == totals


# ---- end to end: a permutation argument ----------------------------------------------------------------

# columns: a, b (pre-random) | t, z (phase 2) | first (public)
A, B, T, Z, FIRST = range(5)


def _permutation_system():
    cset = CS.ConstraintSet([CS.var(FIRST) * (CS.var(Z) - 1), CS.nxt(Z) - CS.var(Z) * CS.var(T)], 2)
    layout = CS.WitnessLayout(columns=5, randoms=1, pre_random_columns=2,
                              public_columns=CS.PublicColumns().first())
    return cset, layout


def _permutation_trace(log_height, spoil):
    r = random.Random(log_height)
    rows = 1 << log_height
    a = [r.randrange(M) for _ in range(rows)]
    b = list(a)
    r.shuffle(b)
    if spoil:
        b[rows // 3] = (b[rows // 3] + 1) % M
    vals = []
    for i in range(rows):
        vals += [a[i], b[i], 11, 13, 17]  # t, z and the strip arrive unwritten
    return CS.Trace(D.to_device(D.ints_to_limbs(vals)), 5)


def _phase2(prover):
    """t = (a + gamma) / (b + gamma) by a fill, z = its running product from 1."""
    g = CS.rand(0)
    prover.fill({T: (CS.var(A) + g) * CS.inv(CS.var(B) + g)})
    return prover.scan([("mul", T, Z, 1)])


@pytest.mark.parametrize("log_height", [6, 10])
def test_permutation_argument_end_to_end(log_height):
    cset, layout = _permutation_system()
    trace = _permutation_trace(log_height, spoil=False)
    tr = Transcript()
    vt, vt2 = tr.clone(), tr.clone()
    prover = CS.System.phased_prover(tr, cset, layout, trace)
    assert prover.shift_columns == [Z]
    assert _phase2(prover) == [1]  # the grand product closes: no (1 - last) gate is needed
    m = D.limbs_to_ints(D.from_device(trace.matrix()))
    gamma, z = prover.randoms[0], 1
    for i in range(1 << log_height):  # the columns the constraints speak of, by hand
        a, b, t = m[5 * i + A], m[5 * i + B], m[5 * i + T]
        assert t * (b + gamma) % M == (a + gamma) % M and m[5 * i + Z] == z
        assert m[5 * i + FIRST] == (i == 0)
        z = z * t % M
    proof = prover.prove(tr, 0, 0)
    # the verifier: no trace, its own spec of the public column
    assert proof.verify(vt, cset, layout, 0, 0, public=CS.PublicColumns().first())
    assert vt.random() == tr.random()
    proof._output[16 * Z] ^= 1
    assert not proof.verify(vt2, cset, layout, 0, 0, public=CS.PublicColumns().first())
    proof._output[16 * Z] ^= 1
    assert proof.verify(vt2, cset, layout, 0, 0, public=CS.PublicColumns().first())


@pytest.mark.parametrize("log_height", [6, 10])
def test_no_permutation_no_closed_product(log_height):
    cset, layout = _permutation_system()
    trace = _permutation_trace(log_height, spoil=True)
    prover = CS.System.phased_prover(Transcript(), cset, layout, trace)
    assert _phase2(prover) != [1]


def test_phased_prover_scan_refuses_committed_and_public_columns():
    cset, layout = _permutation_system()
    trace = _permutation_trace(6, spoil=False)
    prover = CS.System.phased_prover(Transcript(), cset, layout, trace)
    before = D.from_device(trace.matrix()).copy()
    for dst in (A, B, FIRST):
        with pytest.raises(ValueError):
            prover.scan([("mul", T, Z, 1), ("add", T, dst, 0)])
    assert np.array_equal(D.from_device(trace.matrix()), before)
