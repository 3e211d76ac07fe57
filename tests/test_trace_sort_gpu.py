"""mlh_trace_sort on the GPU: sorted copies of columns of a device trace against
the plain-Python model tests/sort_reference.py, under the default launch and
under the shapes of mlh_trace_sort_shaped where the seams are (equal keys
across waves, tiles and blocks, uneven and empty block ranges), up to a memory
log sorted, multiplied up and proved through PhasedProver.  Every comparison is
bit-exact and on the whole matrix, and the number of digit passes is checked
against the byte positions in which the keys differ."""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

import sort_reference as SR
import stream_harness as H
import test_stream_contract_gpu as TSC
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.transcript import Transcript

pytestmark = pytest.mark.gpu

M = SR.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]
NONE = CS.SORT_NO_COLUMN

# (threads, rows per thread, max blocks) of mlh_trace_sort_shaped
SHAPES = [(64, 1, 1),       # many tiles in one block: the running offsets between tiles
          (64, 2, 3),       # uneven ranges and, at small heights, blocks with an empty range
          (128, 4, 2),
          (256, 16, 1024)]
MANY_BLOCKS = (64, 1, 1024)  # one wave and one row per thread: every tile its own block
ALL_PASSES = 1               # flags bit 0


# ---- helpers -----------------------------------------------------------------------------

def _sort(mat, W, keys, copies, perm=None, shape=None):
    """mat: (H * W, 4) uint32 limbs on the host.  -> (the matrix after the call
    as such an array, the digit passes).  shape None: mlh_trace_sort."""
    m = D.to_device(mat)
    passes = CS.Trace(m, W).sort(keys, copies, perm, shape=shape)
    return D.from_device(m), passes


def _column(mat, W, c):
    return D.limbs_to_ints(np.ascontiguousarray(mat.reshape(-1, W, 4)[:, c, :]))


def _model(mat, W, keys, copies, perm=None):
    """The model on the columns the call touches (the others stay as they
    are): -> (the expected matrix as limbs, pi)."""
    a = mat.reshape(-1, W, 4)
    used = sorted(set(keys) | {c for p in copies for c in p} | ({perm} if perm is not None else set()))
    at = {c: k for k, c in enumerate(used)}
    small = D.limbs_to_ints(np.ascontiguousarray(a[:, used, :]))
    out, pi = SR.sort_matrix(small, len(used), [at[k] for k in keys],
                             [(at[s], at[d]) for s, d in copies],
                             None if perm is None else at[perm])
    want = a.copy()
    want[:, used, :] = D.ints_to_limbs(out).reshape(-1, len(used), 4)
    return want.reshape(-1, 4), pi


def _differing_bytes(mat, W, keys):
    """The byte positions, over the key columns, in which not all rows agree:
    the digit passes that cannot be skipped."""
    a = mat.reshape(-1, W, 4)
    n = 0
    for k in keys:
        b = np.ascontiguousarray(a[:, k, :]).view(np.uint8).reshape(-1, 16)
        n += int((b != b[0]).any(axis=0).sum())
    return n


def _check(mat, W, keys, copies, perm, shapes):
    """The model's bytes under every shape of ``shapes`` (None: the default
    launch; a fourth entry: the flags); the passes are the differing bytes, or
    all 16 per key under flags bit 0."""
    want, pi = _model(mat, W, keys, copies, perm)
    need = _differing_bytes(mat, W, keys)
    for shape in shapes:
        got, passes = _sort(mat, W, keys, copies, perm, shape)
        assert np.array_equal(got, want), shape
        forced = shape is not None and len(shape) > 3 and shape[3] & ALL_PASSES
        assert passes == (16 * len(keys) if forced else need), shape
    return want, pi


def _tile_log(shape):
    return (shape[0] * shape[1]).bit_length() - 1


def _default_heights():
    """Around one tile of the default rule, from mlh_trace_sort_launch_info."""
    threads, rows, _ = CS.trace_sort_launch_info(0, 1, 1)
    top = (threads * rows).bit_length() - 1
    return sorted({min(L, 14) for L in (0, 1, 6, top - 1, top, top + 1, top + 3)})


def _with_keys(W, rows, seed, columns):
    """A random matrix whose column c holds columns[c] (a list of ints)."""
    mat = D.random_limbs(W * rows, seed).reshape(rows, W, 4).copy()
    for c, vals in columns.items():
        mat[:, c, :] = D.ints_to_limbs(vals)
    return mat.reshape(-1, 4)


# ---- the default launch ----------------------------------------------------------------------

@pytest.mark.parametrize("log_height", _default_heights())
@pytest.mark.parametrize("width", [2, 3, 8, 32])
def test_default_launch_matches_model(width, log_height):
    """Random 128-bit keys: all 16 digit passes of every key run (one row:
    none)."""
    mat = D.random_limbs(width << log_height, 2000 * width + log_height)
    if width == 2:    # one key and one output
        _check(mat, 2, [0], [], 1, [None])
        _check(mat, 2, [1], [(1, 0)], None, [None])
    elif width == 3:  # the key sorted, and pi
        _check(mat, 3, [1], [(1, 0)], 2, [None])
    else:             # two keys, the second also a source; an untouched rest
        _check(mat, width, [width - 1, 2], [(2, 0), (3, 1), (width - 1, 4)], 5, [None])


def test_default_launch_reaches_one_block_and_several():
    blocks = [CS.trace_sort_launch_info(L, 8, 2)[2] for L in _default_heights()]
    assert blocks[0] == 1 and blocks[-1] > 2


# ---- explicit shapes: the seams ------------------------------------------------------------------

SEAMS = [(shape, L) for shape in SHAPES
         for L in range(_tile_log(shape) - 1, _tile_log(shape) + 4)] + [(MANY_BLOCKS, 12)]


@pytest.mark.parametrize("shape,log_height", SEAMS)
def test_shaped_launch_matches_model_and_default(shape, log_height):
    """From half a tile to 8 tiles, keys of 16 bits (so that equal keys abound
    at every seam) in one column and random ones in a second."""
    W, rows = 5, 1 << log_height
    r = random.Random("seam %r %d" % (shape, log_height))
    mat = _with_keys(W, rows, 88 + log_height, {0: [r.randrange(1 << 16) for _ in range(rows)]})
    _check(mat, W, [0], [(0, 2), (1, 3)], 4, [shape, None])
    _check(mat, W, [1], [(0, 2)], None, [shape, None])


# ---- stability ---------------------------------------------------------------------------------------

STABLE = [(None, 10), (None, 12), ((64, 1, 1024), 8), ((64, 1, 1024, ALL_PASSES), 8),
          ((64, 2, 3), 9), ((64, 2, 3, ALL_PASSES), 9), ((256, 8, 1024, ALL_PASSES), 12),
          ((128, 4, 2, ALL_PASSES), 11)]


@pytest.mark.parametrize("shape,log_height", STABLE)
@pytest.mark.parametrize("n_values", [3, 1])
def test_equal_keys_keep_their_row_order(n_values, shape, log_height):
    """Keys from three values, and from one: pi is the model's -- the identity
    for one value, also through all 16 passes that flags bit 0 forces."""
    W, rows = 3, 1 << log_height
    r = random.Random("stable %d %r" % (n_values, shape))
    values = [r.randrange(M) for _ in range(n_values)]
    mat = _with_keys(W, rows, 5, {0: [r.choice(values) for _ in range(rows)]})
    want, pi = _check(mat, W, [0], [(0, 1)], 2, [shape])
    assert _column(want, W, 2) == pi
    if n_values == 1:
        assert pi == list(range(rows))
        assert _column(want, W, 1) == _column(mat, W, 0)


# ---- every digit alone ---------------------------------------------------------------------------------

@pytest.mark.parametrize("byte", range(16))
def test_keys_that_differ_in_one_byte(byte):
    """2^8 rows whose keys differ in one byte position only: one pass, and the
    model's order."""
    r = random.Random(byte)
    base = r.randrange(1 << 112)  # bytes 14 and 15 zero: every key is canonical
    base &= ~(0xFF << (8 * byte))
    keys = [base | (r.randrange(256) << (8 * byte)) for _ in range(256)]
    assert len(set(keys)) > 1
    mat = _with_keys(3, 256, 40 + byte, {1: keys})
    for shape in (None, (64, 1, 1024), (64, 2, 1)):
        got, passes = _sort(mat, 3, [1], [(1, 0)], 2, shape)
        assert passes == 1
        assert np.array_equal(got, _model(mat, 3, [1], [(1, 0)], 2)[0]), shape


@pytest.mark.parametrize("limb", [1, 2, 3])
def test_keys_across_a_limb_boundary(limb):
    """Keys {x, x + 2^(32 limb) y}: the low limb must not outrank the high one."""
    r = random.Random(limb)
    rows = 1 << 9
    keys = []
    for _ in range(rows):
        x, y = r.randrange(1 << 32), r.randrange(4)
        keys.append(x + (y << (32 * limb)) if r.random() < 0.5 else x)
    mat = _with_keys(2, rows, 60 + limb, {0: keys})
    _check(mat, 2, [0], [(0, 1)], None, [None, (64, 2, 3)])


# ---- skewed digits ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["all but one", "0 and 255", "256 once each"])
def test_skewed_digits(what):
    r = random.Random(what)
    rows = 256 if what == "256 once each" else 1 << 11
    if what == "all but one":
        digits = [7] * rows
        digits[rows // 3] = 200
    elif what == "0 and 255":
        digits = [r.choice((0, 255)) for _ in range(rows)]
    else:
        digits = list(range(256))
        r.shuffle(digits)
    for byte in (0, 5):
        mat = _with_keys(3, rows, 70, {0: [(d << (8 * byte)) + (1 << 100) for d in digits]})
        want, pi = _check(mat, 3, [0], [(0, 1)], 2,
                          [None, (64, 1, 1024), (64, 2, 3), (256, 1, 1, ALL_PASSES)])
        if what == "256 once each":
            assert [digits[i] for i in pi] == list(range(256))


# ---- several keys ----------------------------------------------------------------------------------------

MULTI_SHAPES = [None, (64, 2, 3), (128, 4, 2), MANY_BLOCKS]


def test_address_then_time():
    W, rows = 6, 1 << 10
    r = random.Random("memory")
    addrs = [r.randrange(1 << 32) for _ in range(5)]
    time = list(range(rows))
    r.shuffle(time)
    mat = _with_keys(W, rows, 71, {0: [r.choice(addrs) for _ in range(rows)], 1: time})
    want, pi = _check(mat, W, [0, 1], [(0, 3), (1, 4), (2, 5)], None, MULTI_SHAPES)
    a, t = _column(want, W, 3), _column(want, W, 4)
    assert all((a[i], t[i]) < (a[i + 1], t[i + 1]) for i in range(rows - 1))


def test_four_keys_where_only_the_last_differs():
    W, rows = 6, 1 << 10
    r = random.Random("four")
    const = [r.randrange(M) for _ in range(3)]
    mat = _with_keys(W, rows, 72, {0: [const[0]] * rows, 1: [const[1]] * rows, 2: [const[2]] * rows,
                                   3: [r.randrange(1 << 20) for _ in range(rows)]})
    _check(mat, W, [0, 1, 2, 3], [(3, 4)], 5, MULTI_SHAPES)
    # ... and where the first decides and the others break its ties
    mat = _with_keys(W, rows, 73, {k: [r.randrange(3) for _ in range(rows)] for k in range(4)})
    _check(mat, W, [0, 1, 2, 3], [(3, 4)], 5, MULTI_SHAPES)


def test_the_same_column_as_key_twice():
    W, rows = 3, 1 << 10
    r = random.Random("twice")
    mat = _with_keys(W, rows, 74, {0: [r.randrange(1 << 12) for _ in range(rows)]})
    want, _ = _check(mat, W, [0, 0], [(0, 1)], 2, [None, (64, 2, 3)])
    assert np.array_equal(want, _model(mat, W, [0], [(0, 1)], 2)[0])


# ---- pass skipping ---------------------------------------------------------------------------------------

def test_passes_that_are_skipped_and_passes_that_are_forced():
    W, rows = 3, 1 << 11
    r = random.Random("skip")
    mat = _with_keys(W, rows, 75, {0: [r.randrange(1 << 32) for _ in range(rows)]})
    want = _model(mat, W, [0], [(0, 1)], 2)[0]
    got, passes = _sort(mat, W, [0], [(0, 1)], 2)
    assert passes <= 4 and passes == _differing_bytes(mat, W, [0]) and np.array_equal(got, want)
    got, passes = _sort(mat, W, [0], [(0, 1)], 2, (256, 8, 1024, ALL_PASSES))
    assert passes == 16 and np.array_equal(got, want)
    mat = _with_keys(W, rows, 76, {0: [12345 << 64] * rows})
    got, passes = _sort(mat, W, [0], [(0, 1)], 2)
    assert passes == 0 and np.array_equal(got, _model(mat, W, [0], [(0, 1)], 2)[0])
    assert _column(got, W, 2) == list(range(rows))


# ---- extreme values ----------------------------------------------------------------------------------------

def test_extreme_values():
    W, rows = 3, 1 << 9
    r = random.Random("extreme")
    pool = [0, 1, M - 1, 1 << 127, (1 << 127) + 1, (1 << 64) - 1, 1 << 64]
    mat = _with_keys(W, rows, 77, {0: [r.choice(pool) for _ in range(rows)]})
    want, _ = _check(mat, W, [0], [(0, 1)], 2, [None, (64, 2, 3), MANY_BLOCKS])
    s = _column(want, W, 1)
    assert s == sorted(s) and set(s) == set(pool)


# ---- copies ----------------------------------------------------------------------------------------------

def test_sixteen_copies_at_width_32():
    W, L = 32, 10
    mat = D.random_limbs(W << L, 3232)
    r = random.Random(32)
    dst = r.sample(range(16, 32), 16)
    src = [r.randrange(16) for _ in range(16)]  # sources repeat
    want, _ = _check(mat, W, [3, 9], list(zip(src, dst)), None, [None, (64, 2, 3), (256, 16, 1024)])
    keep = list(range(16))
    assert want.reshape(-1, W, 4)[:, keep, :].tobytes() == mat.reshape(-1, W, 4)[:, keep, :].tobytes()


def test_perm_column_alone_and_a_source_into_two_destinations():
    W, L = 4, 10
    mat = D.random_limbs(W << L, 44)
    _check(mat, W, [2], [], 0, [None, (64, 2, 3)])
    want, _ = _check(mat, W, [2], [(1, 0), (1, 3)], None, [None, (64, 2, 3)])
    assert _column(want, W, 0) == _column(want, W, 3)


# ---- argument errors ---------------------------------------------------------------------------------

_OK = dict(log_height=6, width=6, keys=[0, 1], src=[0, 2], dst=[3, 4], perm=5,
           shape=(256, 8, 1024, 0))
BAD = {
    "width 0": dict(width=0), "width 33": dict(width=33), "log_height 29": dict(log_height=29),
    "no key": dict(keys=[]), "five keys": dict(keys=[0, 1, 0, 1, 0]),
    "seventeen copies": dict(src=[0] * 17, dst=list(range(6, 23)), width=32),
    "no output": dict(src=[], dst=[], perm=NONE),
    "key at width": dict(keys=[0, 6]), "source at width": dict(src=[0, 6]),
    "destination at width": dict(dst=[3, 6]), "perm at width": dict(perm=6),
    "destination twice": dict(dst=[3, 3]), "destination is a key": dict(dst=[3, 1]),
    "destination is a source": dict(dst=[2, 4]), "destination is the perm column": dict(dst=[3, 5]),
    "perm is a key": dict(perm=0), "perm is a source": dict(perm=2),
    "null matrix": dict(matrix=None), "null keys": dict(keys=None), "null sources": dict(src=None),
    "null destinations": dict(dst=None),
    "threads 32": dict(shape=(32, 4, 8, 0)), "threads 512": dict(shape=(512, 4, 8, 0)),
    "threads 96": dict(shape=(96, 4, 8, 0)), "rows 0": dict(shape=(64, 0, 8, 0)),
    "rows 3": dict(shape=(64, 3, 8, 0)), "rows 32": dict(shape=(64, 32, 8, 0)),
    "no block": dict(shape=(64, 4, 0, 0)), "1025 blocks": dict(shape=(64, 4, 1025, 0)),
    "flags 2": dict(shape=(256, 8, 1024, 2)), "flags 3": dict(shape=(256, 8, 1024, 3)),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_errors_leave_the_matrix_alone(what):
    a = dict(_OK, **BAD[what])
    mat = D.random_limbs(32 << 6, 5)  # room for the widest case that could be taken as valid
    m = D.to_device(mat)
    lib, ctx = D.lib(), D.context()
    arr = lambda v: None if v is None else (ctypes.c_uint32 * max(len(v), 1))(*v)
    n_keys = 2 if a["keys"] is None else len(a["keys"])
    n_copies = 2 if a["src"] is None or a["dst"] is None else len(a["src"])
    mp = D.ptr(m) if a.get("matrix", True) is not None else None
    args = (mp, a["log_height"], a["width"], n_keys, arr(a["keys"]), n_copies, arr(a["src"]),
            arr(a["dst"]), a["perm"])
    calls = [lambda p: lib.mlh_trace_sort_shaped(ctx, *args, p, *a["shape"])]
    if a["shape"] == _OK["shape"]:
        calls.append(lambda p: lib.mlh_trace_sort(ctx, *args, p))
    passes = ctypes.c_uint32(77)
    for call in calls:
        for p in (ctypes.byref(passes), None):
            assert call(p) == INVALID, what
            assert lib.mlh_last_error(ctx)
    assert passes.value == 77
    torch.cuda.synchronize()
    assert np.array_equal(D.from_device(m), mat)
    assert lib.mlh_trace_sort(None, *args, None) == INVALID


def test_the_valid_base_of_the_error_cases_is_accepted():
    a = _OK
    mat = D.random_limbs(a["width"] << a["log_height"], 5)
    copies = list(zip(a["src"], a["dst"]))
    _check(mat, a["width"], a["keys"], copies, a["perm"], [None, a["shape"]])


def test_mirror_rejects_before_the_library():
    t = CS.Trace(D.to_device(D.random_limbs(4 << 3, 1)), 4)
    before = D.from_device(t.matrix()).copy()
    for keys, copies, perm in (([0], [], None), ([0], [(1, 0)], None), ([0], [(0, 4)], None),
                               ([0], [(0, 1)], 1), ([0, 1, 2, 3, 0], [(0, 1)], None)):
        with pytest.raises(ValueError):
            t.sort(keys, copies, perm)
    with pytest.raises(_lib.MlhError):
        t.sort([0], [(0, 1)], shape=(96, 1, 1))
    assert np.array_equal(D.from_device(t.matrix()), before)


# ---- scratch poison ----------------------------------------------------------------------------------

def test_scratch_poison_does_not_reach_the_output():
    """The pairs, the census and the tables of a pass come from the pool: under
    two different poison words, on several blocks (some with an empty range),
    the same bytes both times and the model's."""
    W, L = 6, 10
    r = random.Random("poison")
    rows = 1 << L
    mat = _with_keys(W, rows, 606, {0: [r.randrange(7) << 40 for _ in range(rows)],
                                    1: [r.randrange(1 << 20) for _ in range(rows)]})
    want, _ = _model(mat, W, [0, 1], [(0, 2), (1, 3), (5, 4)])
    lib, ctx = D.lib(), D.context()
    results = []
    try:
        for word in (3, 0x01234567):
            for shape in ((64, 2, 3), (64, 1, 1024), (128, 2, 5, ALL_PASSES)):
                D.check(lib.mlh_set_scratch_poison(ctx, word), ctx)
                results.append(_sort(mat, W, [0, 1], [(0, 2), (1, 3), (5, 4)], None, shape))
    finally:
        D.check(lib.mlh_set_scratch_poison(ctx, 0), ctx)
    for got, _ in results:
        assert np.array_equal(got, want)


# ---- the stream contract ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def S():
    return H.side_stream()


def test_sort_with_late_trace(S):
    """The call waits for its census itself: on a busy side stream it sorts the
    trace that arrives late, not what stood in the buffer before."""
    L, W = 10, 5
    a = D.random_limbs(W << L, 323)
    want, _ = _model(a, W, [1, 0], [(0, 2), (1, 3)], 4)

    def call(buf):
        passes = CS.Trace(buf, W).sort([1, 0], [(0, 2), (1, 3)], 4)
        return passes, D.from_device(buf).tobytes()

    TSC._same(TSC._returns(S, "trace_sort (10, 5)", [a], call), (32, want.tobytes()))


def test_sort_behind_pending_work(S):
    """With flags bit 0 the call does not wait: enqueued behind pending work it
    gives the model's bytes."""
    L, W = 10, 5
    a = D.random_limbs(W << L, 324)
    want, _ = _model(a, W, [1], [(0, 2), (1, 3)], 4)

    def op(buf):  # in place
        CS.Trace(buf, W).sort([1], [(0, 2), (1, 3)], 4, shape=(128, 2, 3, ALL_PASSES))
        return buf

    TSC._both(TSC._enqueue(S, "trace_sort, every pass (10, 5)", [a], op), want)


# ---- end to end: a memory log in address-then-time order ---------------------------------------------------

# columns: addr, time, value (pre-random) | their sorted copies, t, z (phase 2) | first (public)
ADDR, TIME, VAL, S_ADDR, S_TIME, S_VAL, T, Z, FIRST = range(9)
LOG_ROWS = 6


def _memory_system():
    gamma, beta = CS.rand(0), CS.rand(1)
    log = CS.tuple_key((ADDR, TIME, VAL), beta)
    srt = CS.tuple_key((S_ADDR, S_TIME, S_VAL), beta)
    cset = CS.ConstraintSet([CS.var(FIRST) * (CS.var(Z) - 1),
                             CS.nxt(Z) * (gamma - srt) - CS.var(Z) * (gamma - log)], 2)
    layout = CS.WitnessLayout(columns=9, randoms=2, pre_random_columns=3,
                              public_columns=CS.PublicColumns().first())
    fill = {T: (gamma - log) * CS.inv(gamma - srt)}
    return cset, layout, fill


@functools.lru_cache(maxsize=None)
def _memory_log():
    r = random.Random("memory log")
    rows = 1 << LOG_ROWS
    time = list(range(rows))
    r.shuffle(time)
    vals = []
    for i in range(rows):
        vals += [r.choice((0x10, 0x14, 0x18, 0xFFFF0000, 1 << 40)), time[i], r.randrange(M),
                 11, 12, 13, 14, 15, 16]  # the sorted copies, t, z and the strip arrive unwritten
    return tuple(vals)


def _memory_prover():
    cset, layout, fill = _memory_system()
    trace = CS.Trace(D.to_device(D.ints_to_limbs(list(_memory_log()))), 9)
    tr = Transcript()
    tr.absorb(b"memory log")
    vt = tr.clone()
    prover = CS.System.phased_prover(tr, cset, layout, trace)
    assert prover.shift_columns == [Z]
    prover.sort([ADDR, TIME], [(ADDR, S_ADDR), (TIME, S_TIME), (VAL, S_VAL)])
    prover.fill(fill)
    total = prover.scan([("mul", T, Z, 1)])
    return prover, trace, tr, vt, total


def test_memory_log_end_to_end():
    cset, layout, _ = _memory_system()
    prover, trace, tr, vt, total = _memory_prover()
    assert total == [1]  # the grand product closes: no (1 - last) gate is needed
    m = D.limbs_to_ints(D.from_device(trace.matrix()))
    want, pi = SR.sort_matrix(list(_memory_log()), 9, [ADDR, TIME],
                              [(ADDR, S_ADDR), (TIME, S_TIME), (VAL, S_VAL)])
    for c in (ADDR, TIME, VAL, S_ADDR, S_TIME, S_VAL):
        assert m[c::9] == want[c::9]
    pairs = list(zip(m[S_ADDR::9], m[S_TIME::9]))
    assert pairs == sorted(pairs) and len(set(pairs)) == len(pairs)
    res, pub = prover.check()
    assert res.ok and res.bad_rows == 0 and pub.ok
    proof = prover.prove(tr, 0, 0)
    assert proof.verify(vt, cset, layout, 0, 0, public=CS.PublicColumns().first())
    assert vt.random() == tr.random()


def test_memory_log_with_a_spoilt_sorted_column():
    cset, layout, _ = _memory_system()
    prover, trace, tr, vt, _ = _memory_prover()
    row = 21
    m = trace.matrix()
    m[row * 9 + S_VAL, 0] ^= 1
    res, _ = prover.check()
    assert not res.ok and res.counts == [0, 1] and res.first_rows == [None, row]
    assert res.first_bad_row == row and res.first_bad_constraint == 1
    proof = prover.prove(tr, 0, 0)
    assert not proof.verify(vt, cset, layout, 0, 0, public=CS.PublicColumns().first())


def test_phased_prover_sort_refuses_committed_and_public_columns():
    cset, layout, _ = _memory_system()
    trace = CS.Trace(D.to_device(D.ints_to_limbs(list(_memory_log()))), 9)
    prover = CS.System.phased_prover(Transcript(), cset, layout, trace)
    before = D.from_device(trace.matrix()).copy()
    for dst in (VAL, FIRST):
        with pytest.raises(ValueError):
            prover.sort([ADDR, TIME], [(ADDR, S_ADDR), (TIME, dst)])
        with pytest.raises(ValueError):
            prover.sort([ADDR, TIME], [(ADDR, S_ADDR)], dst)
    assert np.array_equal(D.from_device(trace.matrix()), before)
