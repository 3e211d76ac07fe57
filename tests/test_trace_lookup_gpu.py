"""A lookup's multiplicities on the GPU: mlh_trace_lookup_counts and its shaped
entry against the plain-Python model tests/lookup_reference.py, up to the
lookup of test_phased_proof_gpu.py proved with its m column counted on the
device.  Every comparison is bit-exact."""
import ctypes
import random

import pytest

import lookup_reference as LR
import test_phased_proof_gpu as TP
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.transcript import Transcript

pytestmark = pytest.mark.gpu

M = D.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]


def _dev(values):
    return D.to_device(D.ints_to_limbs(values))


def _host(t):
    return D.limbs_to_ints(D.from_device(t))


def _mask(cols):
    return sum(1 << c for c in cols)


def _default(m, L, W, values, T, C):
    return CS.Trace(m, W).lookup_counts(values, T, C)


def _shaped(m, L, W, values, T, C, log_slots, hash_bits, max_blocks=0, flags=0):
    ctx = D.context()
    n, first = ctypes.c_uint64(), ctypes.c_uint64()
    st = D.lib().mlh_trace_lookup_counts_shaped(ctx, D.ptr(m), L, W, _mask(values), T, C,
                                                ctypes.byref(n), ctypes.byref(first), log_slots,
                                                hash_bits, max_blocks, flags)
    assert st == 0, D.lib().mlh_last_error(ctx)
    return n.value, (None if first.value == 2 ** 64 - 1 else first.value)


def _check(matrix, L, W, values, T, C, shapes=()):
    """The default entry, then every shape (keyword arguments of _shaped), each
    on a fresh copy: all equal to the model.  Returns the model's result."""
    want = LR.lookup_counts(matrix, W, values, T, C)
    for shape in (None,) + tuple(shapes):
        m = _dev(matrix)
        if shape is None:
            n, first = _default(m, L, W, values, T, C)
        else:
            n, first = _shaped(m, L, W, values, T, C, **shape)
        got = _host(m)
        assert (n, first) == want[1:], shape
        assert got == want[0], shape
        for j in range(W):  # only the count column is written
            if j != C:
                assert got[j::W] == matrix[j::W]
    return want


def _inputs(L, W, values, T, C, dist, seed):
    """Random canonical elements everywhere (the count column included: it is
    overwritten), the value columns drawn from the table column: from its first
    16 entries ("hot", the existing lookup's shape) or from all of it."""
    h = 1 << L
    r = random.Random("%s %d %d %s" % (seed, L, W, dist))
    matrix = [r.randrange(M) for _ in range(h * W)]
    table = matrix[T::W]
    pool = table[:16] if dist == "hot" else table
    for i in range(h):
        for c in values:
            matrix[i * W + c] = pool[r.randrange(len(pool))]
    return matrix


# ---- heights and widths ---------------------------------------------------------------------

# width 3 holds one value column beside T and C; width 5 one or three
LAYOUTS = [(3, (0,), 1, 2), (5, (2,), 0, 4), (5, (0, 2, 4), 1, 3)]
CASES = [(L, W, v, T, C, dist) for L in (0, 1, 6, 8, 9, 12) for (W, v, T, C) in LAYOUTS
         for dist in ("hot", "uniform")]
CASES += [(7, 32, (29,), 30, 31, "uniform"), (7, 32, (29, 3, 17), 30, 31, "hot")]


@pytest.mark.parametrize("L,W,values,T,C,dist", CASES)
def test_counts_match_the_model(L, W, values, T, C, dist):
    matrix = _inputs(L, W, values, T, C, dist, "case")
    out, n, first = _check(matrix, L, W, values, T, C)
    assert (n, first) == (0, None)
    assert sum(out[C::W]) == len(values) << L


# ---- duplicates in the table ------------------------------------------------------------------

@pytest.mark.parametrize("values", [(0,), (0, 2, 4)])
@pytest.mark.parametrize("kind", ["last_quarter", "one_key", "boundaries"])
def test_duplicate_table_entries_lowest_row_owns(kind, values):
    L, W, T, C = 10, 5, 1, 3
    h = 1 << L
    matrix = _inputs(L, W, values, T, C, "uniform", kind)
    if kind == "last_quarter":
        dup = list(range(3 * h // 4, h))
    elif kind == "one_key":
        dup = list(range(h))
    else:
        dup = [0, 255, 256, h - 1]
    key = matrix[dup[0] * W + T]
    lost = {matrix[j * W + T] for j in dup[1:]}  # keys that leave the table
    for j in dup:
        matrix[j * W + T] = key
    for i in range(h):  # values that pointed at a replaced entry follow it
        for c in values:
            if matrix[i * W + c] in lost:
                matrix[i * W + c] = key
    out, n, first = _check(matrix, L, W, values, T, C,
                           shapes=[dict(log_slots=L, hash_bits=L), dict(log_slots=L + 1, hash_bits=0)]
                           if kind != "one_key" else [dict(log_slots=L, hash_bits=L, flags=1)])
    assert (n, first) == (0, None)
    counts = out[C::W]
    assert counts[dup[0]] > 0 and all(counts[j] == 0 for j in dup[1:])
    if kind == "one_key":
        assert counts[0] == len(values) * h


# ---- missing values -----------------------------------------------------------------------------

def _not_in(table, r):
    s = set(table)
    while True:
        v = r.randrange(M)
        if v not in s:
            return v


@pytest.mark.parametrize("values", [(0,), (0, 2, 4)])
@pytest.mark.parametrize("where", ["none", "row0", "last", "several"])
def test_missing_values_are_counted_and_located(where, values):
    L, W, T, C = 9, 5, 1, 3
    h = 1 << L
    matrix = _inputs(L, W, values, T, C, "uniform", where)
    r = random.Random(where)
    rows = {"none": [], "row0": [0], "last": [h - 1], "several": [300, 17, 256, 17, h - 1]}[where]
    for k, i in enumerate(rows):  # (row 17 twice: two pairs of one row when there are 3 columns)
        matrix[i * W + values[k % len(values)]] = _not_in(matrix[T::W], r)
    pairs = len({(i, values[k % len(values)]) for k, i in enumerate(rows)})
    out, n, first = _check(matrix, L, W, values, T, C)
    assert n == pairs and first == (min(rows) if rows else None)
    assert sum(out[C::W]) == (len(values) << L) - pairs


# ---- hash and compare use all 128 bits ---------------------------------------------------------

@pytest.mark.parametrize("limb", range(4))
def test_keys_that_differ_in_one_limb(limb):
    L, W, T, C = 6, 3, 1, 2
    h = 1 << L
    r = random.Random(limb)
    base = [r.randrange(1 << 32) for _ in range(3)] + [0x12345678]
    table = []
    for j in range(h):
        w = list(base)
        w[limb] = (w[limb] + 0x01000193 * (j + 1)) & 0xFFFFFFFF if limb < 3 else j + 1
        table.append(sum(x << (32 * k) for k, x in enumerate(w)))
    assert len(set(table)) == h and max(table) < M
    order = list(range(h))
    r.shuffle(order)
    matrix = [v for i in range(h) for v in (table[order[i]], table[i], 12345)]
    out, n, first = _check(matrix, L, W, (0,), T, C, shapes=[dict(log_slots=L, hash_bits=L)])
    assert out[C::W] == [1] * h and n == 0


# ---- every value equal to one key ----------------------------------------------------------------

def test_one_hot_key_with_and_without_wave_aggregation():
    L, W, values, T, C = 12, 5, (0, 2, 4), 1, 3
    h = 1 << L
    matrix = _inputs(L, W, values, T, C, "uniform", "one")
    owner = 1234
    key = matrix[owner * W + T]
    for i in range(h):
        for c in values:
            matrix[i * W + c] = key
    out, n, first = _check(matrix, L, W, values, T, C,
                           shapes=[dict(log_slots=L + 1, hash_bits=L + 1, flags=1),
                                   dict(log_slots=L + 1, hash_bits=L + 1, flags=0, max_blocks=3)])
    assert out[owner * W + C] == 3 << 12 and sum(out[C::W]) == 3 << 12 and n == 0
    a, b = _dev(matrix), _dev(matrix)
    _shaped(a, L, W, values, T, C, L + 1, L + 1, flags=0)
    _shaped(b, L, W, values, T, C, L + 1, L + 1, flags=1)
    assert _host(a) == _host(b) == out


# ---- shaped probe paths ----------------------------------------------------------------------------

@pytest.mark.parametrize("L", [6, 8])
@pytest.mark.parametrize("shape", ["one_chain", "hash3", "full", "full_missing"])
def test_shaped_probe_paths(L, shape):
    W, values, T, C = 5, (0, 2, 4), 1, 3
    h = 1 << L
    matrix = _inputs(L, W, values, T, C, "uniform", shape)
    assert len(set(matrix[T::W])) == h  # distinct keys: log_slots = L is a full table
    shapes = {"one_chain": [dict(log_slots=L + 1, hash_bits=0), dict(log_slots=L, hash_bits=0)],
              "hash3": [dict(log_slots=L + 1, hash_bits=3), dict(log_slots=L, hash_bits=3)],
              "full": [dict(log_slots=L, hash_bits=L), dict(log_slots=L, hash_bits=L, flags=1)],
              "full_missing": [dict(log_slots=L, hash_bits=L), dict(log_slots=L, hash_bits=0),
                               dict(log_slots=L, hash_bits=3)]}[shape]
    rows = [5, h - 1, 33] if shape == "full_missing" else []
    r = random.Random(shape)
    for k, i in enumerate(rows):  # no empty slot ends these probes: the bound does
        matrix[i * W + values[k]] = _not_in(matrix[T::W], r)
    out, n, first = _check(matrix, L, W, values, T, C, shapes=shapes)
    assert (n, first) == ((3, 5) if rows else (0, None))


@pytest.mark.parametrize("max_blocks", [1, 2])
def test_grid_stride_loop(max_blocks):
    L, W, values, T, C = 10, 5, (0, 2, 4), 1, 3
    matrix = _inputs(L, W, values, T, C, "hot", "stride")
    matrix[777 * W + 2] = _not_in(matrix[T::W], random.Random(1))
    out, n, first = _check(matrix, L, W, values, T, C,
                           shapes=[dict(log_slots=L + 1, hash_bits=L + 1, max_blocks=max_blocks),
                                   dict(log_slots=L + 1, hash_bits=L + 1, max_blocks=max_blocks,
                                        flags=1)])
    assert (n, first) == (1, 777)


# ---- one moderate shape -----------------------------------------------------------------------------

def test_many_blocks_and_real_collisions():
    L, W, values, T, C = 16, 5, (0,), 1, 3
    assert CS.lookup_counts_launch_info(L, 1) == (256, 256, L + 2)
    matrix = _inputs(L, W, values, T, C, "uniform", "moderate")
    out, n, first = _check(matrix, L, W, values, T, C,
                           shapes=[dict(log_slots=L + 2, hash_bits=L + 2),
                                   dict(log_slots=L + 1, hash_bits=L + 1)])
    assert (n, first) == (0, None) and sum(out[C::W]) == 1 << L


# ---- argument errors ----------------------------------------------------------------------------------

def test_argument_errors_leave_the_matrix_unchanged():
    lib, ctx = D.lib(), D.context()
    L, W = 3, 5
    matrix = _inputs(L, W, (0,), 1, 3, "uniform", "args")
    m = _dev(matrix)
    n, first = ctypes.c_uint64(), ctypes.c_uint64()
    rn, rf = ctypes.byref(n), ctypes.byref(first)
    f, s = lib.mlh_trace_lookup_counts, lib.mlh_trace_lookup_counts_shaped
    p = D.ptr(m)
    bad = [
        (p, L, W, 0, 1, 3, rn, rf),          # empty mask
        (p, L, W, 1 << 5, 1, 3, rn, rf),     # a mask bit at the width
        (p, L, W, 1 | 1 << 31, 1, 3, rn, rf),
        (p, L, W, 1, 5, 3, rn, rf),          # T at the width
        (p, L, W, 1, 1, 5, rn, rf),          # C at the width
        (p, L, W, 1, 3, 3, rn, rf),          # T == C
        (p, L, W, 0b11, 1, 3, rn, rf),       # T in the mask
        (p, L, W, 0b1001, 1, 3, rn, rf),     # C in the mask
        (None, L, W, 1, 1, 3, rn, rf),       # NULL pointers
        (p, L, W, 1, 1, 3, None, rf),
        (p, L, W, 1, 1, 3, rn, None),
        (p, L, 0, 1, 1, 3, rn, rf),          # width 0 and 33
        (p, L, 33, 1, 1, 3, rn, rf),
        (p, 29, W, 1, 1, 3, rn, rf),         # log_height above 28
    ]
    for args in bad:
        assert f(ctx, *args) == INVALID, args
        assert s(ctx, *args, L + 2, L + 2, 0, 0) == INVALID, args
    assert f(None, p, L, W, 1, 1, 3, rn, rf) == INVALID
    ok = (p, L, W, 1, 1, 3, rn, rf)
    assert s(ctx, *ok, L - 1, 0, 0, 0) == INVALID       # log_slots < log_height
    assert s(ctx, *ok, 32, 3, 0, 0) == INVALID          # log_slots > 31
    assert s(ctx, *ok, L + 1, L + 2, 0, 0) == INVALID   # hash_bits > log_slots
    assert s(ctx, *ok, L + 1, L + 1, 0, 2) == INVALID   # an unknown flag
    assert s(ctx, *ok, L + 1, L + 1, 0, 3) == INVALID
    assert _host(m) == matrix
    assert s(ctx, *ok, L, L, 7, 1) == 0, lib.mlh_last_error(ctx)
    assert _host(m) == LR.lookup_counts(matrix, W, (0,), 1, 3)[0]
    with pytest.raises(ValueError):
        CS.Trace(m, W).lookup_counts([0], 1, 1)


def test_calling_twice_gives_the_same_bytes():
    L, W, values, T, C = 9, 5, (0, 4), 1, 3
    matrix = _inputs(L, W, values, T, C, "hot", "twice")
    m = _dev(matrix)
    trace = CS.Trace(m, W)
    assert trace.lookup_counts(values, T, C) == (0, None)
    once = _host(m)
    assert once == LR.lookup_counts(matrix, W, values, T, C)[0]
    assert trace.lookup_counts(values, T, C) == (0, None)
    assert _host(m) == once  # overwritten, not accumulated


# ---- the lookup, end to end ---------------------------------------------------------------------------

COL_A, COL_T, COL_M, COL_U, COL_V = range(5)


def _lookup_matrix():
    h = 1 << TP.LOOKUP_L
    a, t, mult = TP._lookup_inputs(False)
    r = random.Random("garbage")
    return a, t, mult, [v for i in range(h) for v in (a[i], t[i], r.randrange(M), 0, 0)]


def test_lookup_proof_with_multiplicities_counted_on_the_device():
    a, t, mult, values = _lookup_matrix()
    matrix = _dev(values)
    cset, layout = TP._lookup_system()
    trace = CS.Trace(matrix, 5)
    assert trace.lookup_multiplicities([COL_A], COL_T, COL_M) is None
    assert _host(matrix)[COL_M::5] == mult
    tr = Transcript()
    tr.absorb(b"lookup")
    vt = tr.clone()
    prover = CS.System.phased_prover(tr, cset, layout, trace)
    prover.fill({COL_U: CS.inv(CS.rand(0) - CS.var(COL_A)),
                 COL_V: -CS.var(COL_M) * CS.inv(CS.rand(0) - CS.var(COL_T))})
    proof = prover.prove(tr, 0)
    assert prover.column_sum == 0
    assert proof.verify(vt, cset, layout, 0, 0)
    assert vt.random() == tr.random()
    old, ovt, _, _, old_colsum = TP._lookup_prove(bump=False)
    assert old_colsum == 0 and old.verify(ovt, cset, layout, 0, 0)
    assert proof.sumcheck_polynomials == old.sumcheck_polynomials
    assert proof.output == old.output
    assert proof.commitments == old.commitments
    assert tr.random() == ovt.random()


def test_lookup_multiplicities_names_the_row_of_a_value_outside_the_table():
    a, t, mult, values = _lookup_matrix()
    assert 1 not in t
    values[37 * 5 + COL_A] = 1
    matrix = _dev(values)
    trace = CS.Trace(matrix, 5)
    with pytest.raises(ValueError, match="row 37"):
        trace.lookup_multiplicities([COL_A], COL_T, COL_M)
    assert trace.lookup_counts([COL_A], COL_T, COL_M) == (1, 37)
    want = list(mult)
    want[t.index(a[37])] -= 1
    assert _host(matrix)[COL_M::5] == want
