"""Host side of a lookup's multiplicities (no GPU): the plain-Python model
tests/lookup_reference.py on hand-written cases, the argument checks of the
Python mirror, the three C symbols and the launch rule stated in
include/mlhip.h."""
import ctypes
import os
import re

import pytest
import torch

import lookup_reference as LR
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS

INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mlhip.h")


# ---- the model ---------------------------------------------------------------------------

def _matrix(rows):
    return [v for row in rows for v in row]


def test_model_counts_one_value_column():
    # columns: a, t, m
    rows = [[5, 5, 99], [7, 6, 99], [5, 7, 99], [5, 8, 99]]
    out, n, first = LR.lookup_counts(_matrix(rows), 3, [0], 1, 2)
    assert out == _matrix([[5, 5, 3], [7, 6, 0], [5, 7, 1], [5, 8, 0]])
    assert (n, first) == (0, None)


def test_model_lowest_duplicate_owns_the_count():
    rows = [[4, 9, 1], [9, 4, 1], [9, 9, 1], [4, 4, 1]]  # table 9, 4, 9, 4
    out, n, first = LR.lookup_counts(_matrix(rows), 3, [0], 1, 2)
    assert out[2::3] == [2, 2, 0, 0]
    assert (n, first) == (0, None)
    rows = [[3, 3, 0]] * 4  # one key throughout
    out, _, _ = LR.lookup_counts(_matrix(rows), 3, [0], 1, 2)
    assert out[2::3] == [4, 0, 0, 0]


def test_model_missing_values():
    rows = [[1, 1, 0], [8, 2, 0], [2, 3, 0], [9, 4, 0]]
    out, n, first = LR.lookup_counts(_matrix(rows), 3, [0], 1, 2)
    assert out[2::3] == [1, 1, 0, 0] and (n, first) == (2, 1)
    assert out[0::3] == [1, 8, 2, 9] and out[1::3] == [1, 2, 3, 4]  # only the count column


def test_model_several_value_columns_count_pairs():
    # columns: a0, t, a1, m, a2; width 5
    rows = [[1, 1, 2, 7, 2], [2, 2, 2, 7, 50], [1, 3, 3, 7, 1], [60, 3, 60, 7, 3]]
    out, n, first = LR.lookup_counts(_matrix(rows), 5, [0, 2, 4], 1, 3)
    assert out[3::5] == [3, 4, 2, 0]  # 1: rows 0, 2, 2; 2: rows 0, 0, 1, 1; 3: rows 2, 3
    assert (n, first) == (3, 1)  # 50 in row 1, 60 twice in row 3
    assert 3 + 4 + 2 + n == 4 * 3


def test_model_large_elements_compare_whole():
    hi = 1 << 96
    rows = [[hi + 1, 1, 0], [1, hi + 1, 0]]
    out, n, first = LR.lookup_counts(_matrix(rows), 3, [0], 1, 2)
    assert out[2::3] == [1, 1] and n == 0


# ---- the mirror's argument checks ----------------------------------------------------------

def _trace(h=8, W=5):
    return CS.Trace(torch.zeros((h * W, 4), dtype=torch.int32), W)


@pytest.mark.parametrize("values,table,count", [
    ([], 1, 2),          # no value column
    ([5], 1, 2),         # a value column at the width
    ([-1], 1, 2),
    ([0], 5, 2),         # the table column at the width
    ([0], 1, 5),         # the count column at the width
    ([0], -1, 2),
    ([0], 2, 2),         # table == count
    ([0, 1], 1, 2),      # the table column among the values
    ([0, 2], 1, 2),      # the count column among the values
])
@pytest.mark.parametrize("method", ["lookup_counts", "lookup_multiplicities"])
def test_mirror_rejects_columns_before_touching_the_library(method, values, table, count):
    with pytest.raises(ValueError):
        getattr(_trace(), method)(values, table, count)


# ---- the C ABI ---------------------------------------------------------------------------

NAMES = ["mlh_trace_lookup_counts", "mlh_trace_lookup_counts_launch_info",
         "mlh_trace_lookup_counts_shaped"]
_CTYPE = {"uint32_t": ctypes.c_uint32, "uint64_t*": ctypes.POINTER(ctypes.c_uint64),
          "uint32_t*": ctypes.POINTER(ctypes.c_uint32), "mlh_ctx*": ctypes.c_void_p,
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


@pytest.mark.parametrize("log_height", [0, 8, 20, 22])
@pytest.mark.parametrize("n_values", [1, 3])
def test_launch_info_follows_the_rule_in_the_header(log_height, n_values):
    """256 threads, min(ceil(rows * value columns / 256), 1024) blocks, and
    log_height + 2 slot bits."""
    threads, blocks, log_slots = CS.lookup_counts_launch_info(log_height, n_values)
    work = n_values << log_height
    assert threads == 256
    assert blocks == min(-(-work // 256), 1024)
    assert log_slots == log_height + 2


def test_launch_info_argument_errors():
    f = _lib.load().mlh_trace_lookup_counts_launch_info
    t, b, s = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    r = ctypes.byref
    assert f(29, 1, r(t), r(b), r(s)) == INVALID
    assert f(8, 0, r(t), r(b), r(s)) == INVALID
    assert f(8, 31, r(t), r(b), r(s)) == INVALID
    assert f(8, 1, None, r(b), r(s)) == INVALID
    assert f(8, 1, r(t), None, r(s)) == INVALID
    assert f(8, 1, r(t), r(b), None) == INVALID
    assert f(28, 30, r(t), r(b), r(s)) == 0 and (t.value, b.value, s.value) == (256, 1024, 30)


def test_null_context_and_pointers_are_invalid_without_a_device():
    lib = _lib.load()
    n, first = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.mlh_trace_lookup_counts(None, None, 3, 3, 1, 1, 2, ctypes.byref(n),
                                       ctypes.byref(first)) == INVALID
