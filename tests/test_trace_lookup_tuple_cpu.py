"""Host side of a tuple lookup's multiplicities (no GPU): the plain-Python model
tests/lookup_tuple_reference.py on hand-written cases, the argument checks of
the Python mirror, the three C symbols and the launch rule stated in
include/mlhip.h, and ``tuple_key`` through the host interpreter of fill
programs."""
import ctypes
import os
import random
import re

import pytest
import torch

import lookup_tuple_reference as LT
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd.device import M

INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mlhip.h")


# ---- the model ---------------------------------------------------------------------------

def _matrix(rows):
    return [v for row in rows for v in row]


def test_model_component_wise_trap():
    # columns: a, b, c, ta, tb, tc, m.  Every component of (3, 5, 7) occurs in
    # its own table column, the triple in no table row.
    rows = [[3, 5, 7, 3, 1, 2, 9], [3, 1, 2, 4, 5, 6, 9], [4, 5, 6, 8, 9, 7, 9], [8, 9, 7, 0, 0, 0, 9]]
    out, n, first = LT.lookup_tuple_counts(_matrix(rows), 7, [(0, 1, 2)], (3, 4, 5), 6)
    assert out[6::7] == [1, 1, 1, 0]
    assert (n, first) == (1, 0)
    for j in range(6):  # only the count column is written
        assert out[j::7] == _matrix(rows)[j::7]


def test_model_permuted_tuples_are_different_keys():
    # columns: x, y, tx, ty, m.  (1, 2) is a key, (2, 1) is not.
    rows = [[1, 2, 1, 2, 0], [2, 1, 5, 5, 0], [1, 2, 6, 6, 0], [5, 5, 7, 7, 0]]
    out, n, first = LT.lookup_tuple_counts(_matrix(rows), 5, [(0, 1)], (2, 3), 4)
    assert out[4::5] == [2, 1, 0, 0] and (n, first) == (1, 1)
    # the table read in the other order: key(0) = (2, 1)
    out, n, first = LT.lookup_tuple_counts(_matrix(rows), 5, [(0, 1)], (3, 2), 4)
    assert out[4::5] == [1, 1, 0, 0] and (n, first) == (2, 0)


def test_model_lowest_duplicate_owns_the_count():
    # rows 0 and 2 hold the key (4, 9); rows 1 and 3 agree with it in one component only
    rows = [[4, 9, 4, 9, 1], [4, 9, 4, 8, 1], [4, 8, 4, 9, 1], [3, 9, 3, 9, 1]]
    out, n, first = LT.lookup_tuple_counts(_matrix(rows), 5, [(0, 1)], (2, 3), 4)
    assert out[4::5] == [2, 1, 0, 1] and (n, first) == (0, None)


def test_model_disabled_pair_is_neither_counted_nor_missing():
    # columns: x, y, tx, ty, m, s
    rows = [[1, 1, 1, 1, 0, 1], [9, 9, 2, 2, 0, 0], [2, 2, 3, 3, 0, 0], [8, 8, 4, 4, 0, 5]]
    m = _matrix(rows)
    out, n, first = LT.lookup_tuple_counts(m, 6, [(0, 1)], (2, 3), 4, selectors=[5])
    assert out[4::6] == [1, 0, 0, 0] and (n, first) == (1, 3)
    out, n, first = LT.lookup_tuple_counts(m, 6, [(0, 1)], (2, 3), 4, selectors=[None])
    assert out[4::6] == [1, 1, 0, 0] and (n, first) == (2, 1)
    assert LT.lookup_tuple_counts(m, 6, [(0, 1)], (2, 3), 4)[1:] == (2, 1)


def test_model_shared_value_columns():
    # columns: x, y, z, tx, ty, tz, m: an AND table, looked up as (x, y, z) and (y, x, z)
    table = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 1)]
    vals = [(0, 1, 0), (1, 1, 1), (1, 0, 0), (1, 0, 0)]
    rows = [list(v) + list(t) + [77] for v, t in zip(vals, table)]
    out, n, first = LT.lookup_tuple_counts(_matrix(rows), 7, [(0, 1, 2), (1, 0, 2)], (3, 4, 5), 6)
    assert out[6::7] == [0, 3, 3, 2] and (n, first) == (0, None)


def test_model_at_arity_one_is_the_one_column_model():
    import lookup_reference as LR
    r = random.Random(1)
    W, h = 5, 32
    m = [r.randrange(8) for _ in range(W * h)]
    want = LR.lookup_counts(m, W, [0, 2, 4], 1, 3)
    assert LT.lookup_tuple_counts(m, W, [(0,), (2,), (4,)], (1,), 3) == want


# ---- the mirror's argument checks ----------------------------------------------------------

def _trace(h=8, W=12):
    return CS.Trace(torch.zeros((h * W, 4), dtype=torch.int32), W)


@pytest.mark.parametrize("tuples,table,count,selectors", [
    ([], (3, 4), 6, None),                       # no tuple
    ([(0, 1)] * 17, (3, 4), 6, None),            # 17 tuples
    ([(0, 1)], (), 6, None),                     # arity 0
    ([(0,) * 9], tuple(range(1, 10)), 11, None),  # arity 9
    ([(0, 1, 2, 3, 4)] * 7, (5, 6, 7, 8, 9), 11, None),  # 35 value columns
    ([(0, 1)], (3, 12), 6, None),                # a table column at the width
    ([(0, 1)], (3, -1), 6, None),
    ([(0, 1)], (3, 3), 6, None),                 # two equal table columns
    ([(0, 1)], (3, 4), 12, None),                # the count column at the width
    ([(0, 1)], (3, 4), -1, None),
    ([(0, 1)], (3, 6), 6, None),                 # the count column among the table columns
    ([(0, 6)], (3, 4), 6, None),                 # ... among the values
    ([(0, 1)], (3, 4), 6, [6]),                  # ... as a selector
    ([(0, 12)], (3, 4), 6, None),                # a value column at the width
    ([(0, -1)], (3, 4), 6, None),
    ([(0, 3)], (3, 4), 6, None),                 # a value column that is a table column
    ([(0, 1, 2)], (3, 4), 6, None),              # a tuple of another arity
    ([(0, 1), (2,)], (3, 4), 6, None),
    ([(0, 1)], (3, 4), 6, [12]),                 # a selector at the width
    ([(0, 1)], (3, 4), 6, [-1]),
    ([(0, 1)], (3, 4), 6, [5, 5]),               # two selectors for one tuple
    ([(0, 1), (1, 0)], (3, 4), 6, [5]),
])
@pytest.mark.parametrize("method", ["lookup_tuple_counts", "lookup_tuple_multiplicities"])
def test_mirror_rejects_columns_before_touching_the_library(method, tuples, table, count, selectors):
    with pytest.raises(ValueError):
        getattr(_trace(), method)(tuples, table, count, selectors)


def test_mirror_accepts_what_the_header_allows():
    """Repeated value columns within and across tuples, a selector that is a
    value or a table column, None among the selectors: the lists as the C
    entry takes them."""
    arity, n, table, values, sels = CS._lookup_tuple_lists(
        12, [(0, 0, 1), (1, 0, 0)], (3, 5, 4), 6, [None, 3])
    assert (arity, n) == (3, 2)
    assert list(table) == [3, 5, 4] and list(values) == [0, 0, 1, 1, 0, 0]
    assert list(sels) == [0xFFFFFFFF, 3]
    assert CS._lookup_tuple_lists(12, [(0,)], (1,), 2, None)[4] is None
    assert CS._lookup_tuple_lists(32, [tuple(range(8))] * 4, tuple(range(8, 16)), 31, None)[:2] == (8, 4)
    assert CS._lookup_tuple_lists(32, [(0, 1)] * 16, (2, 3), 4, None)[:2] == (2, 16)


# ---- the C ABI ---------------------------------------------------------------------------

NAMES = ["mlh_trace_lookup_tuple_counts", "mlh_trace_lookup_tuple_counts_launch_info",
         "mlh_trace_lookup_tuple_counts_shaped"]
_CTYPE = {"uint32_t": ctypes.c_uint32, "uint64_t*": ctypes.POINTER(ctypes.c_uint64),
          "uint32_t*": ctypes.POINTER(ctypes.c_uint32),
          "const uint32_t*": ctypes.POINTER(ctypes.c_uint32), "mlh_ctx*": ctypes.c_void_p,
          "void*": ctypes.c_void_p}


def _header_argtypes(name):
    text = open(HEADER).read()
    m = re.search(r"mlh_status\s+%s\(([^)]*)\);" % name, text)
    assert m, "%s is not declared in include/mlhip.h" % name
    return [_CTYPE[" ".join(p.split()[:-1])] for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_symbols_exist_with_the_declared_signatures(name):
    lib = _lib.load()
    fn = getattr(lib, name)  # AttributeError when libmlhip.so lacks the symbol
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int
    assert args == _header_argtypes(name)
    assert list(fn.argtypes) == args


def test_shaped_entry_takes_the_first_entrys_arguments_then_four():
    a, s = _header_argtypes(NAMES[0]), _header_argtypes(NAMES[2])
    assert s == a + [ctypes.c_uint32] * 4


def test_header_constants():
    text = open(HEADER).read()
    for name, value in (("MLH_LOOKUP_MAX_ARITY", "8"), ("MLH_LOOKUP_MAX_TUPLES", "16"),
                        ("MLH_LOOKUP_NO_SELECTOR", "0xFFFFFFFFu")):
        assert re.search(r"#define\s+%s\s+%s\s" % (name, value), text), name
    assert (CS.LOOKUP_MAX_ARITY, CS.LOOKUP_MAX_TUPLES, CS.LOOKUP_NO_SELECTOR) == (8, 16, 0xFFFFFFFF)


@pytest.mark.parametrize("log_height", [0, 8, 20, 22])
@pytest.mark.parametrize("n_tuples", [1, 3])
def test_launch_info_follows_the_rule_in_the_header(log_height, n_tuples):
    """256 threads, min(ceil(rows * tuples / 256), 1024) blocks, and log_height
    + 2 slot bits."""
    threads, blocks, log_slots = CS.lookup_tuple_counts_launch_info(log_height, n_tuples)
    work = n_tuples << log_height
    assert threads == 256
    assert blocks == min(-(-work // 256), 1024)
    assert log_slots == log_height + 2


def test_launch_info_argument_errors():
    f = _lib.load().mlh_trace_lookup_tuple_counts_launch_info
    t, b, s = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    r = ctypes.byref
    assert f(29, 1, r(t), r(b), r(s)) == INVALID
    assert f(8, 0, r(t), r(b), r(s)) == INVALID
    assert f(8, 17, r(t), r(b), r(s)) == INVALID
    assert f(8, 1, None, r(b), r(s)) == INVALID
    assert f(8, 1, r(t), None, r(s)) == INVALID
    assert f(8, 1, r(t), r(b), None) == INVALID
    assert f(28, 16, r(t), r(b), r(s)) == 0 and (t.value, b.value, s.value) == (256, 1024, 30)


def test_null_context_and_pointers_are_invalid_without_a_device():
    lib = _lib.load()
    n, first = ctypes.c_uint64(), ctypes.c_uint64()
    cols = (ctypes.c_uint32 * 2)(0, 1)
    assert lib.mlh_trace_lookup_tuple_counts(None, None, 3, 3, 1, cols, 1, cols, None, 2,
                                             ctypes.byref(n), ctypes.byref(first)) == INVALID


# ---- tuple_key ---------------------------------------------------------------------------

@pytest.mark.parametrize("arity", [1, 2, 3, 8])
def test_tuple_key_through_the_fill_interpreter(arity):
    """Column W - 1 := tuple_key(columns, rand(1)), compiled by compile_fill and
    run by the host interpreter, against sum_k alpha^k * row[columns[k]]."""
    W = 12
    r = random.Random(arity)
    cols = r.sample(range(W - 1), arity)  # unsorted
    prog = CS.FillProgram(CS.compile_fill({W - 1: CS.tuple_key(cols, CS.rand(1))}, W, 2))
    assert prog.n_inverses == 0 and prog.output_mask == 1 << (W - 1)
    edge = [0, 1, M - 1]
    for trial in range(4):
        row = [edge[(trial + j) % 3] if trial < 2 else r.randrange(M) for j in range(W)]
        gamma, alpha = r.randrange(M), (M - 1 if trial == 0 else r.randrange(M))
        want = sum(pow(alpha, k, M) * row[c] for k, c in enumerate(cols)) % M
        out = prog.evaluate(row, [gamma, alpha])
        assert out[W - 1] == want
        assert out[:W - 1] == row[:W - 1]


def test_tuple_key_with_an_integer_and_in_an_inverse():
    W = 5
    e = CS.tuple_key((2, 0), 7)
    prog = CS.FillProgram(CS.compile_fill({4: CS.inv(CS.rand(0) - e)}, W, 1))
    row, gamma = [11, 0, 5, 0, 0], 1000
    assert prog.evaluate(row, [gamma])[4] == pow(gamma - (5 + 7 * 11), M - 2, M)
    with pytest.raises(ValueError):
        CS.tuple_key((), 7)
