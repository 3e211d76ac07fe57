"""mlh_trace_scan without a GPU: the three entries as include/mlhip.h declares
them, the launch rule of mlh_trace_scan_launch_info, the Python mirror's own
argument checks, and the plain-Python model tests/scan_reference.py against
hand-written cases."""
import ctypes
import os
import re

import pytest

import scan_reference as SR
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS

M = SR.M
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "mlhip.h")
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]

NAMES = ["mlh_trace_scan", "mlh_trace_scan_launch_info", "mlh_trace_scan_shaped"]
_CTYPE = {"uint32_t": ctypes.c_uint32, "uint32_t*": ctypes.POINTER(ctypes.c_uint32),
          "mlh_ctx*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const uint8_t*": ctypes.c_void_p,
          "uint8_t*": ctypes.c_void_p}


def _header_argtypes(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"mlh_status\s+%s\(([^)]*)\);" % name, text)
    assert m, "%s is not declared in include/mlhip.h" % name
    return [_CTYPE[" ".join(p.split()[:-1])] for p in m.group(1).split(",")]


# ---- the C ABI ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_header_declares_the_entry_and_the_library_has_it(name):
    lib = _lib.load()
    fn = getattr(lib, name)  # AttributeError when libmlhip.so lacks the symbol
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int
    assert args == _header_argtypes(name)
    assert list(fn.argtypes) == args


def test_header_defines_the_ops_and_shaped_adds_three_arguments():
    text = open(HEADER).read()
    assert re.search(r"#define\s+MLH_SCAN_ADD\s+0\b", text)
    assert re.search(r"#define\s+MLH_SCAN_MUL\s+1\b", text)
    assert CS.SCAN_OPS == {"add": 0, "mul": 1}
    assert _header_argtypes(NAMES[2]) == _header_argtypes(NAMES[0]) + [ctypes.c_uint32] * 3


@pytest.mark.parametrize("log_height", [0, 10, 20, 22, 32])
@pytest.mark.parametrize("width,n_scans", [(1, 1), (8, 2), (32, 8)])
def test_launch_info_follows_the_rule_in_the_header(log_height, width, n_scans):
    """256 threads, 4 consecutive rows per thread, min(ceil(2^log_height /
    1024), 1024) blocks."""
    threads, rows, blocks = CS.trace_scan_launch_info(log_height, width, n_scans)
    assert (threads, rows) == (256, 4)
    assert blocks == min(-(-(1 << log_height) // (threads * rows)), 1024)


def test_launch_info_argument_errors():
    f = _lib.load().mlh_trace_scan_launch_info
    t, r, b = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
    out = (ctypes.byref(t), ctypes.byref(r), ctypes.byref(b))
    assert f(10, 4, 1, *out) == 0
    for log_height, width, n_scans in ((10, 0, 1), (10, 33, 1), (10, 4, 0), (10, 4, 9), (33, 4, 1)):
        t.value = r.value = b.value = 7
        assert f(log_height, width, n_scans, *out) == INVALID
        assert (t.value, r.value, b.value) == (7, 7, 7)
    assert f(10, 4, 1, None, ctypes.byref(r), ctypes.byref(b)) == INVALID
    assert f(10, 4, 1, ctypes.byref(t), None, ctypes.byref(b)) == INVALID
    assert f(10, 4, 1, ctypes.byref(t), ctypes.byref(r), None) == INVALID
    with pytest.raises(Exception):
        CS.trace_scan_launch_info(10, 33, 1)


# ---- the mirror's own checks (nothing reaches the library) ------------------------------------

@pytest.mark.parametrize("scans", [
    [],
    [("add", 0, 1, 0)] * 2,                          # two scans write column 1
    [("add", 0, c, 0) for c in range(4)] * 3,        # 12 scans
    [("max", 0, 1, 0)],
    [("add", 4, 1, 0)],
    [("mul", 0, 4, 1)],
    [("mul", -1, 0, 1)],
])
def test_scan_arrays_rejects(scans):
    with pytest.raises(ValueError):
        CS._scan_arrays(scans, 4)


def test_scan_arrays_accepts_shared_sources_and_chains():
    ops, src, dst, inits = CS._scan_arrays([("mul", 0, 0, 1), ("add", 0, 1, 5), ("add", 1, 2, M - 1)],
                                           4)
    assert (ops, src, dst, inits) == ([1, 0, 0], [0, 0, 1], [0, 1, 2], [1, 5, M - 1])


# ---- the model against cases written out by hand --------------------------------------------

def test_model_running_sum_by_hand():
    # one column: t = 5, 7, 11, 13; z = 100, 105, 112, 123; total 136
    out, totals = SR.scan_matrix([5, 7, 11, 13], 1, [("add", 0, 0, 100)])
    assert out == [100, 105, 112, 123] and totals == [136]
    # the sum wraps: (M - 1) + 2 = 1
    out, totals = SR.scan_matrix([2, 0, 0, M - 3], 1, [("add", 0, 0, M - 1)])
    assert out == [M - 1, 1, 1, 1] and totals == [M - 2]


def test_model_running_product_by_hand():
    # columns (t, z): t = 2, 3, 5, 7 -> z = 1, 2, 6, 30, total 210; t is not written
    m = [2, 9, 3, 9, 5, 9, 7, 9]
    out, totals = SR.scan_matrix(m, 2, [("mul", 0, 1, 1)])
    assert out == [2, 1, 3, 2, 5, 6, 7, 30] and totals == [210]
    # (M - 1)^2 = 1
    out, totals = SR.scan_matrix([M - 1] * 4, 1, [("mul", 0, 0, 3)])
    assert out == [3, M - 3, 3, M - 3] and totals == [3]


def test_model_zero_in_a_product_scan():
    # a zero at row 1: rows 0 and 1 hold what came before it, all after is zero
    out, totals = SR.scan_matrix([4, 0, 6, 7], 1, [("mul", 0, 0, 5)])
    assert out == [5, 20, 0, 0] and totals == [0]
    # a zero at the last row shows in the total only
    out, totals = SR.scan_matrix([4, 2, 3, 0], 1, [("mul", 0, 0, 1)])
    assert out == [1, 4, 8, 24] and totals == [0]


def test_model_snapshot_semantics_by_hand():
    """Two scans in one call, the second reading the column the first writes:
    it sees the values of entry."""
    m = [1, 10, 2, 20, 3, 30, 4, 40]  # columns (x, y)
    out, totals = SR.scan_matrix(m, 2, [("add", 0, 1, 0), ("add", 1, 0, 0)])
    # y <- prefix sums of x: 0 1 3 6 (total 10); x <- prefix sums of the old y: 0 10 30 60 (100)
    assert out == [0, 0, 10, 1, 30, 3, 60, 6] and totals == [10, 100]
