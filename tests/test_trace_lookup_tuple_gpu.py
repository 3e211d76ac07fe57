"""A tuple lookup's multiplicities on the GPU: mlh_trace_lookup_tuple_counts and
its shaped entry against the plain-Python model tests/lookup_tuple_reference.py,
up to a 4-bit XOR lookup proved as a phased system with its m column counted on
the device.  Every comparison is bit-exact, and every column but the count
column is compared byte for byte."""
import ctypes
import random

import pytest

import lookup_tuple_reference as LT
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.transcript import Transcript

pytestmark = pytest.mark.gpu

M = D.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]
NO_SEL = CS.LOOKUP_NO_SELECTOR


def _dev(values):
    return D.to_device(D.ints_to_limbs(values))


def _host(t):
    return D.limbs_to_ints(D.from_device(t))


def _default(m, L, W, tuples, table, C, selectors=None):
    return CS.Trace(m, W).lookup_tuple_counts(tuples, table, C, selectors)


def _shaped(m, L, W, tuples, table, C, selectors=None, log_slots=None, hash_bits=None,
            max_blocks=0, flags=0):
    ctx = D.context()
    arity, n_tuples, tab, vals, sels = CS._lookup_tuple_lists(W, tuples, table, C, selectors)
    n, first = ctypes.c_uint64(), ctypes.c_uint64()
    st = D.lib().mlh_trace_lookup_tuple_counts_shaped(
        ctx, D.ptr(m), L, W, arity, tab, n_tuples, vals, sels, C, ctypes.byref(n),
        ctypes.byref(first), log_slots, hash_bits, max_blocks, flags)
    assert st == 0, D.lib().mlh_last_error(ctx)
    return n.value, (None if first.value == 2 ** 64 - 1 else first.value)


def _check(matrix, L, W, tuples, table, C, selectors=None, shapes=(), default=True):
    """The default entry, then every shape (keyword arguments of _shaped), each
    on a fresh copy: all equal to the model.  Returns the model's result."""
    assert len(matrix) == W << L
    want = LT.lookup_tuple_counts(matrix, W, tuples, table, C, selectors)
    for shape in ((None,) if default else ()) + tuple(shapes):
        m = _dev(matrix)
        if shape is None:
            n, first = _default(m, L, W, tuples, table, C, selectors)
        else:
            n, first = _shaped(m, L, W, tuples, table, C, selectors, **shape)
        got = _host(m)
        assert (n, first) == want[1:], shape
        assert got == want[0], shape
        for j in range(W):  # only the count column is written
            if j != C:
                assert got[j::W] == matrix[j::W]
    return want


def _layout(arity, n_tuples, spare=1, seed=0):
    """(W, tuples, table, C): disjoint columns in a shuffled (unsorted,
    non-adjacent) order, `spare` columns that take no part."""
    W = arity * (n_tuples + 1) + 1 + spare
    cols = list(range(W))
    random.Random("layout %d %d %d" % (arity, n_tuples, seed)).shuffle(cols)
    table = tuple(cols[1:1 + arity])
    tuples = [tuple(cols[1 + arity * (l + 1):1 + arity * (l + 2)]) for l in range(n_tuples)]
    return W, tuples, table, cols[0]


def _key(matrix, W, j, cols):
    return tuple(matrix[j * W + c] for c in cols)


def _put(matrix, W, i, cols, key):
    for c, v in zip(cols, key):
        matrix[i * W + c] = v


def _inputs(L, W, tuples, table, dist, seed):
    """Random canonical elements everywhere (the count column included: it is
    overwritten), every value tuple a copy of a table row's key: of one of the
    first 16 rows ("hot") or of any row."""
    h = 1 << L
    r = random.Random("%s %d %d %s" % (seed, L, W, dist))
    matrix = [r.randrange(M) for _ in range(h * W)]
    pool = min(h, 16) if dist == "hot" else h
    for i in range(h):
        for t in tuples:
            _put(matrix, W, i, t, _key(matrix, W, r.randrange(pool), table))
    return matrix


def _absent(r, arity):
    """A tuple of random elements: no key of a random table but by a 2^-128 accident."""
    return tuple(r.randrange(M) for _ in range(arity))


# ---- 1. model parity ---------------------------------------------------------------------------

CASES = [(L, arity, n, dist) for L in (0, 1, 6, 8, 9, 12) for arity in (1, 2, 3) for n in (1, 3)
         for dist in ("uniform", "hot")]


@pytest.mark.parametrize("L,arity,n_tuples,dist", CASES)
def test_counts_match_the_model(L, arity, n_tuples, dist):
    W, tuples, table, C = _layout(arity, n_tuples)
    matrix = _inputs(L, W, tuples, table, dist, "case")
    out, n, first = _check(matrix, L, W, tuples, table, C)
    assert (n, first) == (0, None)
    assert sum(out[C::W]) == n_tuples << L


def test_one_wave_spans_three_tuples():
    """L = 1: pairs 0..5 of one wave belong to tuples 0, 0, 1, 1, 2, 2; one of
    them is missing, one disabled."""
    L, (W, tuples, table, C) = 1, _layout(2, 3, spare=2)
    matrix = _inputs(L, W, tuples, table, "uniform", "span")
    sel = [c for c in range(W) if c != C and c not in table and all(c not in t for t in tuples)][0]
    matrix[0 * W + sel], matrix[1 * W + sel] = 0, 1
    _put(matrix, W, 1, tuples[1], _absent(random.Random(5), 2))
    _put(matrix, W, 0, tuples[2], _absent(random.Random(6), 2))  # disabled: not missing
    out, n, first = _check(matrix, L, W, tuples, table, C, selectors=[None, None, sel])
    assert (n, first) == (1, 1) and sum(out[C::W]) == 4


def test_arity_eight_width_32_unsorted_table_columns():
    L, W, C = 8, 32, 31
    table = (29, 3, 17, 30, 1, 8, 22, 11)
    rest = [c for c in range(W) if c not in table and c != C]
    random.Random("arity 8").shuffle(rest)
    tuples = [tuple(rest[:8]), tuple(rest[8:16])]
    matrix = _inputs(L, W, tuples, table, "uniform", "arity8")
    r = random.Random(8)
    _put(matrix, W, 77, tuples[1], _absent(r, 8))
    # a tuple that equals a key in seven components and differs in the last
    k = list(_key(matrix, W, 5, table))
    k[7] ^= 1
    _put(matrix, W, 200, tuples[0], k)
    out, n, first = _check(matrix, L, W, tuples, table, C,
                           shapes=[dict(log_slots=L, hash_bits=L), dict(log_slots=L + 1, hash_bits=0)])
    assert (n, first) == (2, 77) and sum(out[C::W]) == (2 << L) - 2


# ---- 2. arity 1 against the one-column entry ---------------------------------------------------------

def test_arity_one_equals_the_one_column_entry():
    L, W, values, T, C = 9, 5, (0, 2, 4), 1, 3
    tuples = [(c,) for c in values]
    matrix = _inputs(L, W, tuples, (T,), "hot", "arity1")
    r = random.Random(1)
    for i, c in ((300, 2), (17, 4), (17, 0)):
        matrix[i * W + c] = r.randrange(M)
    a, b = _dev(matrix), _dev(matrix)
    got_a = CS.Trace(a, W).lookup_counts(values, T, C)
    got_b = CS.Trace(b, W).lookup_tuple_counts(tuples, (T,), C)
    assert got_a == got_b == (3, 17)
    assert _host(a) == _host(b) == LT.lookup_tuple_counts(matrix, W, tuples, (T,), C)[0]


# ---- 3. the component-wise trap, on the XOR table -----------------------------------------------------

XL, XW = 8, 7
A, B, Cc, TA, TB, TC, MM = range(7)


def _xor_matrix(seed, m_garbage=True):
    """2^8 rows (a, b, c, ta, tb, tc, m): the table is every (x, y, x ^ y) of
    4-bit x, y in a shuffled order, the values are random 4-bit pairs with
    their XOR, m is garbage."""
    r = random.Random(seed)
    table = [(x, y, x ^ y) for x in range(16) for y in range(16)]
    r.shuffle(table)
    rows = []
    for j in range(1 << XL):
        x, y = r.randrange(16), r.randrange(16)
        rows.append([x, y, x ^ y, *table[j], r.randrange(M) if m_garbage else 0])
    return [v for row in rows for v in row]


def test_component_wise_trap():
    matrix = _xor_matrix("trap")
    a, b = matrix[37 * XW + A], matrix[37 * XW + B]
    matrix[37 * XW + Cc] = (a ^ b) ^ 5  # still 0..15, still in column tc, but no row's triple
    for col, tcol in ((A, TA), (B, TB), (Cc, TC)):  # per column nothing is missing
        assert set(matrix[col::XW]) <= set(matrix[tcol::XW])
    out, n, first = _check(matrix, XL, XW, [(A, B, Cc)], (TA, TB, TC), MM)
    assert (n, first) == (1, 37)
    table = [_key(matrix, XW, j, (TA, TB, TC)) for j in range(1 << XL)]
    vals = [_key(matrix, XW, i, (A, B, Cc)) for i in range(1 << XL)]
    assert out[MM::XW] == [vals.count(t) for t in table]
    with pytest.raises(ValueError, match="1 looked-up tuple not in .* row 37"):
        CS.Trace(_dev(matrix), XW).lookup_tuple_multiplicities([(A, B, Cc)], (TA, TB, TC), MM)


# ---- 4. order matters -----------------------------------------------------------------------------------

def test_permuted_tuples_are_different_keys():
    """Table rows 2k = (p, q) and 2k + 1 = (q, p); value row i looks up table
    row 5 i + 3 mod h.  hash_bits = 0: every key starts at slot 0 and only the
    comparison tells (p, q) from (q, p)."""
    L, W = 6, 5  # x, y, tx, ty, m
    h = 1 << L
    r = random.Random("order")
    matrix = [0] * (h * W)
    for k in range(h // 2):
        p, q = r.randrange(M), r.randrange(M)
        _put(matrix, W, 2 * k, (2, 3), (p, q))
        _put(matrix, W, 2 * k + 1, (2, 3), (q, p))
    for i in range(h):
        _put(matrix, W, i, (0, 1), _key(matrix, W, (5 * i + 3) % h, (2, 3)))
        matrix[i * W + 4] = r.randrange(M)
    out, n, first = _check(matrix, L, W, [(0, 1)], (2, 3), 4,
                           shapes=[dict(log_slots=L + 2, hash_bits=0), dict(log_slots=L, hash_bits=0)])
    assert out[4::W] == [1] * h and (n, first) == (0, None)
    # the value tuples read in the other order hit the partner rows
    out, n, first = _check(matrix, L, W, [(1, 0)], (2, 3), 4, default=False,
                           shapes=[dict(log_slots=L + 1, hash_bits=0)])
    assert out[4::W] == [1] * h and n == 0
    both = _check(matrix, L, W, [(0, 1), (1, 0)], (2, 3), 4, default=False,
                  shapes=[dict(log_slots=L + 1, hash_bits=0)])
    assert both[0][4::W] == [2] * h


# ---- 5. keys that differ in one limb of one component ----------------------------------------------------

@pytest.mark.parametrize("comp", range(3))
@pytest.mark.parametrize("limb", range(4))
def test_keys_that_differ_in_one_limb_of_one_component(comp, limb):
    L, W = 6, 7  # v0 v1 v2 t0 t1 t2 m
    h = 1 << L
    r = random.Random(4 * comp + limb)
    base = [[r.randrange(1 << 32) for _ in range(3)] + [0x12345678] for _ in range(3)]
    keys = []
    for j in range(h):
        w = [list(x) for x in base]
        w[comp][limb] = (w[comp][limb] + 0x01000193 * (j + 1)) & 0xFFFFFFFF if limb < 3 else j + 1
        keys.append(tuple(sum(x << (32 * k) for k, x in enumerate(e)) for e in w))
    assert len(set(keys)) == h and max(max(k) for k in keys) < M
    order = list(range(h))
    r.shuffle(order)
    matrix = [v for i in range(h) for v in (*keys[order[i]], *keys[i], 12345)]
    out, n, first = _check(matrix, L, W, [(0, 1, 2)], (3, 4, 5), 6,
                           shapes=[dict(log_slots=L + 2, hash_bits=0), dict(log_slots=L, hash_bits=0)])
    assert out[6::W] == [1] * h and n == 0


# ---- 6. partial duplicates and owners ----------------------------------------------------------------------

def _grouped_inputs(L, W, tuples, table, seed):
    """Table keys (g, g', unique): rows agree in all but the last component in
    groups of eight."""
    h = 1 << L
    r = random.Random(seed)
    matrix = [r.randrange(M) for _ in range(h * W)]
    for j in range(h):
        g = random.Random("group %d" % (j // 8))
        _put(matrix, W, j, table[:-1], [g.randrange(M) for _ in table[:-1]])
    assert len({_key(matrix, W, j, table) for j in range(h)}) == h
    for i in range(h):
        for t in tuples:
            _put(matrix, W, i, t, _key(matrix, W, r.randrange(h), table))
    return matrix


def test_rows_that_agree_in_all_but_the_last_component_own_separate_counts():
    L, (W, tuples, table, C) = 9, _layout(3, 2)
    h = 1 << L
    matrix = _grouped_inputs(L, W, tuples, table, "partial")
    assert len({_key(matrix, W, j, table[:2]) for j in range(h)}) == h // 8
    out, n, first = _check(matrix, L, W, tuples, table, C,
                           shapes=[dict(log_slots=L, hash_bits=L), dict(log_slots=L + 1, hash_bits=3)])
    assert (n, first) == (0, None)
    assert sum(1 for c in out[C::W] if c) > h // 2  # spread over the rows, not one per group


@pytest.mark.parametrize("kind", ["last_quarter", "boundaries"])
def test_duplicate_keys_lowest_row_owns(kind):
    L, (W, tuples, table, C) = 9, _layout(3, 2, seed=1)
    h = 1 << L
    matrix = _grouped_inputs(L, W, tuples, table, kind)
    dup = list(range(3 * h // 4, h)) if kind == "last_quarter" else [0, 255, 256, h - 1]
    key = _key(matrix, W, dup[0], table)
    lost = {_key(matrix, W, j, table) for j in dup[1:]}  # keys that leave the table
    for j in dup:
        _put(matrix, W, j, table, key)
    for i in range(h):  # values that pointed at a replaced key follow it
        for t in tuples:
            if _key(matrix, W, i, t) in lost:
                _put(matrix, W, i, t, key)
    out, n, first = _check(matrix, L, W, tuples, table, C,
                           shapes=[dict(log_slots=L, hash_bits=L), dict(log_slots=L + 1, hash_bits=3)])
    assert (n, first) == (0, None)
    counts = out[C::W]
    assert counts[dup[0]] >= len(dup) // 2 and all(counts[j] == 0 for j in dup[1:])
    assert sum(counts) == 2 * h


# ---- 7. selectors ---------------------------------------------------------------------------------------------

def _selector_case(seed):
    """L = 8, three tuples of arity 2 with the selector columns s0, s1, s2."""
    L, (W, tuples, table, C) = 8, _layout(2, 3, spare=3, seed=7)
    used = set(table) | {C} | {c for t in tuples for c in t}
    sels = [c for c in range(W) if c not in used]
    matrix = _inputs(L, W, tuples, table, "hot", seed)
    return L, W, tuples, table, C, sels, matrix


def test_all_zero_selectors_count_nothing_and_miss_nothing():
    L, W, tuples, table, C, sels, matrix = _selector_case("zero")
    r = random.Random(0)
    for i in range(1 << L):
        for s in sels:
            matrix[i * W + s] = 0
        _put(matrix, W, i, tuples[i % 3], _absent(r, 2))  # would be missing
    out, n, first = _check(matrix, L, W, tuples, table, C, selectors=sels)
    assert (n, first) == (0, None) and out[C::W] == [0] * (1 << L)


def test_all_one_selectors_equal_the_call_without_selectors():
    L, W, tuples, table, C, sels, matrix = _selector_case("one")
    for i in range(1 << L):
        for s in sels:
            matrix[i * W + s] = 1
    matrix[9 * W + tuples[1][0]] = 12345  # one missing pair
    with_sel = _check(matrix, L, W, tuples, table, C, selectors=sels)
    without = _check(matrix, L, W, tuples, table, C)
    assert with_sel == without and with_sel[1:] == (1, 9)


def test_mixed_selectors_only_enabled_pairs_are_missing():
    L, W, tuples, table, C, sels, matrix = _selector_case("mixed")
    h = 1 << L
    r = random.Random("mixed")
    enabled_missing, disabled = 0, 0
    for i in range(h):
        for l, s in enumerate(sels):
            on = r.randrange(3) != 0
            # a nonzero selector is any nonzero 16 bytes: 1, M - 1, or only the top bit
            matrix[i * W + s] = r.choice([1, M - 1, 1 << 127]) if on else 0
            if r.randrange(4) == 0 or not on and r.randrange(2):
                _put(matrix, W, i, tuples[l], _absent(r, 2))
                enabled_missing += on
            disabled += not on
    assert enabled_missing and disabled > enabled_missing
    out, n, first = _check(matrix, L, W, tuples, table, C, selectors=sels,
                           shapes=[dict(log_slots=L, hash_bits=L), dict(log_slots=L + 1, hash_bits=0),
                                   dict(log_slots=L + 2, hash_bits=L + 2, flags=1)])
    assert n == enabled_missing
    assert sum(out[C::W]) == 3 * h - disabled - enabled_missing


def test_a_selector_of_two_to_the_127_enables():
    L, W, tuples, table, C, sels, matrix = _selector_case("top bit")
    h = 1 << L
    for i in range(h):
        for s in sels:
            matrix[i * W + s] = 0
    matrix[100 * W + sels[0]] = 1 << 127   # only limb 3 is nonzero
    matrix[101 * W + sels[1]] = 1 << 64    # only limb 2
    matrix[102 * W + sels[2]] = 1 << 32    # only limb 1
    out, n, first = _check(matrix, L, W, tuples, table, C, selectors=sels)
    assert sum(out[C::W]) == 3 and n == 0


def test_no_selector_for_one_tuple_of_three():
    L, W, tuples, table, C, sels, matrix = _selector_case("none of three")
    h = 1 << L
    for i in range(h):
        matrix[i * W + sels[0]] = i & 1
        matrix[i * W + sels[2]] = 0
    out, n, first = _check(matrix, L, W, tuples, table, C, selectors=[sels[0], None, sels[2]])
    assert sum(out[C::W]) == h // 2 + h and n == 0
    # MLH_LOOKUP_NO_SELECTOR itself through the C entry
    m = _dev(matrix)
    ctx = D.context()
    arity, n_t, tab, vals, _ = CS._lookup_tuple_lists(W, tuples, table, C, None)
    raw = (ctypes.c_uint32 * 3)(sels[0], NO_SEL, sels[2])
    cn, cf = ctypes.c_uint64(), ctypes.c_uint64()
    assert D.lib().mlh_trace_lookup_tuple_counts(ctx, D.ptr(m), L, W, arity, tab, n_t, vals, raw, C,
                                                 ctypes.byref(cn), ctypes.byref(cf)) == 0
    assert _host(m) == out and (cn.value, cf.value) == (0, 2 ** 64 - 1)


# ---- 8. shared value columns -------------------------------------------------------------------------------------

def test_shared_value_columns_against_a_commutative_table():
    matrix = _xor_matrix("shared")
    tuples = [(A, B, Cc), (B, A, Cc)]
    out, n, first = _check(matrix, XL, XW, tuples, (TA, TB, TC), MM,
                           shapes=[dict(log_slots=XL, hash_bits=XL)])
    assert (n, first) == (0, None) and sum(out[MM::XW]) == 2 << XL
    table = [_key(matrix, XW, j, (TA, TB, TC)) for j in range(1 << XL)]
    vals = [_key(matrix, XW, i, t) for i in range(1 << XL) for t in tuples]
    assert out[MM::XW] == [vals.count(t) for t in table]


# ---- 9. probe paths and loops -----------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [6, 8])
@pytest.mark.parametrize("shape", ["one_chain", "hash3", "full", "full_missing"])
def test_shaped_probe_paths(L, shape):
    W, tuples, table, C = _layout(2, 3)
    h = 1 << L
    matrix = _inputs(L, W, tuples, table, "uniform", shape)
    assert len({_key(matrix, W, j, table) for j in range(h)}) == h  # log_slots = L: a full table
    shapes = {"one_chain": [dict(log_slots=L + 1, hash_bits=0), dict(log_slots=L, hash_bits=0)],
              "hash3": [dict(log_slots=L + 1, hash_bits=3), dict(log_slots=L, hash_bits=3)],
              "full": [dict(log_slots=L, hash_bits=L), dict(log_slots=L, hash_bits=L, flags=1)],
              "full_missing": [dict(log_slots=L, hash_bits=L), dict(log_slots=L, hash_bits=0),
                               dict(log_slots=L, hash_bits=3)]}[shape]
    rows = [5, h - 1, 33] if shape == "full_missing" else []
    r = random.Random(shape)
    for k, i in enumerate(rows):  # no empty slot ends these probes: the bound does
        _put(matrix, W, i, tuples[k], _absent(r, 2))
    out, n, first = _check(matrix, L, W, tuples, table, C, shapes=shapes)
    assert (n, first) == ((3, 5) if rows else (0, None))


@pytest.mark.parametrize("max_blocks", [1, 2])
def test_grid_stride_loop(max_blocks):
    L, (W, tuples, table, C) = 10, _layout(2, 3)
    matrix = _inputs(L, W, tuples, table, "hot", "stride")
    _put(matrix, W, 777, tuples[1], _absent(random.Random(1), 2))
    out, n, first = _check(matrix, L, W, tuples, table, C, default=False,
                           shapes=[dict(log_slots=L + 1, hash_bits=L + 1, max_blocks=max_blocks),
                                   dict(log_slots=L + 1, hash_bits=L + 1, max_blocks=max_blocks,
                                        flags=1)])
    assert (n, first) == (1, 777)


def test_one_hot_tuple_with_and_without_wave_aggregation():
    L, (W, tuples, table, C) = 12, _layout(2, 3)
    h = 1 << L
    matrix = _inputs(L, W, tuples, table, "uniform", "one")
    owner = 1234
    key = _key(matrix, W, owner, table)
    for i in range(h):
        for t in tuples:
            _put(matrix, W, i, t, key)
    out, n, first = _check(matrix, L, W, tuples, table, C,
                           shapes=[dict(log_slots=L + 1, hash_bits=L + 1, flags=1),
                                   dict(log_slots=L + 1, hash_bits=L + 1, flags=0, max_blocks=3)])
    assert out[owner * W + C] == 3 << 12 and sum(out[C::W]) == 3 << 12 and n == 0


def test_many_blocks_under_the_rule():
    L, (W, tuples, table, C) = 16, _layout(3, 2, spare=0)
    assert CS.lookup_tuple_counts_launch_info(L, 2) == (256, 512, L + 2)
    matrix = _inputs(L, W, tuples, table, "uniform", "moderate")
    out, n, first = _check(matrix, L, W, tuples, table, C)
    assert (n, first) == (0, None) and sum(out[C::W]) == 2 << L


# ---- 10. argument errors -----------------------------------------------------------------------------------------

def test_argument_errors_leave_the_matrix_unchanged():
    lib, ctx = D.lib(), D.context()
    L, W = 3, 12
    tuples, table, C = [(0, 1), (2, 0)], (3, 4), 6
    matrix = _inputs(L, W, tuples, table, "uniform", "args")
    m = _dev(matrix)
    n, first = ctypes.c_uint64(), ctypes.c_uint64()
    rn, rf = ctypes.byref(n), ctypes.byref(first)
    f, s = lib.mlh_trace_lookup_tuple_counts, lib.mlh_trace_lookup_tuple_counts_shaped
    p = D.ptr(m)
    u = lambda *v: (ctypes.c_uint32 * len(v))(*v)
    T, V, S = u(3, 4), u(0, 1, 2, 0), u(5, NO_SEL)
    big_t, big_v = u(*range(12, 21)), u(*range(9))
    bad = [
        (None, L, W, 2, T, 2, V, S, C, rn, rf),        # NULL pointers
        (p, L, W, 2, None, 2, V, S, C, rn, rf),
        (p, L, W, 2, T, 2, None, S, C, rn, rf),
        (p, L, W, 2, T, 2, V, S, C, None, rf),
        (p, L, W, 2, T, 2, V, S, C, rn, None),
        (p, L, 0, 2, T, 2, V, S, C, rn, rf),           # width 0 and 33
        (p, L, 33, 2, T, 2, V, S, C, rn, rf),
        (p, 29, W, 2, T, 2, V, S, C, rn, rf),          # log_height above 28
        (p, L, W, 0, T, 2, V, S, C, rn, rf),           # arity 0 and 9
        (p, L, 32, 9, big_t, 1, big_v, None, 31, rn, rf),
        (p, L, W, 2, T, 0, V, S, C, rn, rf),           # no tuple, 17 tuples
        (p, L, W, 2, T, 17, u(*([0, 1] * 17)), None, C, rn, rf),
        (p, L, W, 5, u(7, 8, 9, 10, 11), 7, u(*([0, 1, 2, 3, 4] * 7)), None, C, rn, rf),  # 35 columns
        (p, L, W, 2, u(3, 12), 2, V, S, C, rn, rf),    # a table column at the width
        (p, L, W, 2, u(3, 3), 2, V, S, C, rn, rf),     # two equal table columns
        (p, L, W, 2, T, 2, u(0, 1, 2, 12), S, C, rn, rf),   # a value column at the width
        (p, L, W, 2, T, 2, u(0, 1, 2, 4), S, C, rn, rf),    # a value column that is a table column
        (p, L, W, 2, T, 2, V, u(5, 12), C, rn, rf),    # a selector at the width
        (p, L, W, 2, T, 2, V, S, 12, rn, rf),          # the count column at the width
        (p, L, W, 2, T, 2, V, S, 4, rn, rf),           # ... a table column
        (p, L, W, 2, T, 2, V, S, 2, rn, rf),           # ... a value column
        (p, L, W, 2, T, 2, V, S, 5, rn, rf),           # ... a selector
    ]
    for args in bad:
        assert f(ctx, *args) == INVALID, args
        assert s(ctx, *args, L + 2, L + 2, 0, 0) == INVALID, args
    assert f(None, p, L, W, 2, T, 2, V, S, C, rn, rf) == INVALID
    ok = (p, L, W, 2, T, 2, V, S, C, rn, rf)
    assert s(ctx, *ok, L - 1, 0, 0, 0) == INVALID       # log_slots < log_height
    assert s(ctx, *ok, 32, 3, 0, 0) == INVALID          # log_slots > 31
    assert s(ctx, *ok, L + 1, L + 2, 0, 0) == INVALID   # hash_bits > log_slots
    assert s(ctx, *ok, L + 1, L + 1, 0, 2) == INVALID   # an unknown flag
    assert s(ctx, *ok, L + 1, L + 1, 0, 3) == INVALID
    assert _host(m) == matrix
    assert s(ctx, *ok, L, L, 7, 1) == 0, lib.mlh_last_error(ctx)
    assert _host(m) == LT.lookup_tuple_counts(matrix, W, tuples, table, C, [5, None])[0]
    with pytest.raises(ValueError):
        CS.Trace(m, W).lookup_tuple_counts(tuples, table, 4)


def test_calling_twice_gives_the_same_bytes():
    L, (W, tuples, table, C) = 9, _layout(3, 2)
    matrix = _inputs(L, W, tuples, table, "hot", "twice")
    m = _dev(matrix)
    trace = CS.Trace(m, W)
    assert trace.lookup_tuple_counts(tuples, table, C) == (0, None)
    once = _host(m)
    assert once == LT.lookup_tuple_counts(matrix, W, tuples, table, C)[0]
    assert trace.lookup_tuple_counts(tuples, table, C) == (0, None)
    assert _host(m) == once  # overwritten, not accumulated


# ---- 11. the XOR lookup, end to end ---------------------------------------------------------------------------------

COL_U, COL_V = 7, 8


def _xor_system():
    gamma, alpha = CS.rand(0), CS.rand(1)
    key_a, key_t = CS.tuple_key((A, B, Cc), alpha), CS.tuple_key((TA, TB, TC), alpha)
    cset = CS.ConstraintSet([CS.var(COL_U) * (gamma - key_a) - 1,
                             CS.var(COL_V) * (gamma - key_t) + CS.var(MM)], 2)
    layout = CS.WitnessLayout(columns=9, randoms=2, pre_random_columns=7,
                              sum_columns=(COL_U, COL_V))
    fill = {COL_U: CS.inv(gamma - key_a), COL_V: -CS.var(MM) * CS.inv(gamma - key_t)}
    return cset, layout, fill


def _xor_trace(host_m):
    """The 2^8 x 9 XOR lookup: m written from the Python model on the host, or
    garbage for the device to count."""
    seven = _xor_matrix("end to end")
    if host_m:
        seven = LT.lookup_tuple_counts(seven, XW, [(A, B, Cc)], (TA, TB, TC), MM)[0]
    return [v for i in range(1 << XL) for v in (*seven[i * XW:(i + 1) * XW], 0, 0)]


def _xor_prove(values, count_on_device):
    cset, layout, fill = _xor_system()
    matrix = _dev(values)
    trace = CS.Trace(matrix, 9)
    if count_on_device:
        assert trace.lookup_tuple_multiplicities([(A, B, Cc)], (TA, TB, TC), MM) is None
    tr = Transcript()
    tr.absorb(b"xor lookup")
    vt = tr.clone()
    prover = CS.System.phased_prover(tr, cset, layout, trace)
    gamma, alpha = prover.randoms
    host = _host(matrix)
    for i in range(1 << XL):  # no zero denominator for this seed
        for cols in ((A, B, Cc), (TA, TB, TC)):
            x, y, z = (host[i * 9 + c] for c in cols)
            assert (gamma - (x + alpha * (y + alpha * z))) % M
    prover.fill(fill)
    proof = prover.prove(tr, 0)
    return proof, prover.column_sum, tr, vt, _host(matrix)


def test_xor_lookup_proof_with_multiplicities_counted_on_the_device():
    cset, layout, _ = _xor_system()
    proof, colsum, tr, vt, filled = _xor_prove(_xor_trace(host_m=False), count_on_device=True)
    assert filled[MM::9] == _xor_trace(host_m=True)[MM::9]
    assert colsum == 0
    assert proof.verify(vt, cset, layout, 0, 0)
    assert vt.random() == tr.random()
    old, old_colsum, otr, ovt, old_filled = _xor_prove(_xor_trace(host_m=True), count_on_device=False)
    assert old_colsum == 0 and old.verify(ovt, cset, layout, 0, 0)
    assert filled == old_filled
    assert proof.sumcheck_polynomials == old.sumcheck_polynomials
    assert proof.output == old.output
    assert proof.commitments == old.commitments
    assert tr.random() == otr.random()


def test_xor_lookup_multiplicities_names_the_row_of_a_wrong_xor():
    values = _xor_trace(host_m=False)
    values[37 * 9 + Cc] ^= 5
    trace = CS.Trace(_dev(values), 9)
    with pytest.raises(ValueError, match="1 looked-up tuple not in .* row 37"):
        trace.lookup_tuple_multiplicities([(A, B, Cc)], (TA, TB, TC), MM)
    assert trace.lookup_tuple_counts([(A, B, Cc)], (TA, TB, TC), MM) == (1, 37)
