"""mlh_trace_sort without a GPU: the three entries as include/mlhip.h declares
them, the launch rule of mlh_trace_sort_launch_info, the Python mirror's own
argument checks, and the plain-Python model tests/sort_reference.py against
hand-written cases."""
import ctypes
import os
import re

import pytest

import sort_reference as SR
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS

M = SR.M
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "mlhip.h")
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]

NAMES = ["mlh_trace_sort", "mlh_trace_sort_launch_info", "mlh_trace_sort_shaped"]
_U32P = ctypes.POINTER(ctypes.c_uint32)
_CTYPE = {"uint32_t": ctypes.c_uint32, "uint32_t*": _U32P, "const uint32_t*": _U32P,
          "mlh_ctx*": ctypes.c_void_p, "void*": ctypes.c_void_p}


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


def test_header_defines_the_limits_and_shaped_adds_four_arguments():
    text = open(HEADER).read()
    assert re.search(r"#define\s+MLH_SORT_MAX_KEYS\s+4\b", text)
    assert re.search(r"#define\s+MLH_SORT_MAX_COPIES\s+16\b", text)
    assert re.search(r"#define\s+MLH_SORT_NO_COLUMN\s+0xFFFFFFFFu\b", text)
    assert (CS.SORT_MAX_KEYS, CS.SORT_MAX_COPIES, CS.SORT_NO_COLUMN) == (4, 16, 0xFFFFFFFF)
    assert _header_argtypes(NAMES[2]) == _header_argtypes(NAMES[0]) + [ctypes.c_uint32] * 4


@pytest.mark.parametrize("log_height", [0, 11, 12, 20, 28])
@pytest.mark.parametrize("width,n_keys", [(1, 1), (8, 2), (32, 4)])
def test_launch_info_follows_the_rule_in_the_header(log_height, width, n_keys):
    """256 threads, 8 rows per thread, min(ceil(2^log_height / 2048), 1024)
    blocks."""
    threads, rows, blocks = CS.trace_sort_launch_info(log_height, width, n_keys)
    assert (threads, rows) == (256, 8)
    assert blocks == min(-(-(1 << log_height) // 2048), 1024)
    text = " ".join(open(HEADER).read().split())
    assert ("threads per block (256), rows per thread (8) and blocks * (min(ceil(2^log_height / "
            "(threads * rows_per_thread)), 1024))") in text


def test_launch_info_argument_errors():
    f = _lib.load().mlh_trace_sort_launch_info
    t, r, b = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
    out = (ctypes.byref(t), ctypes.byref(r), ctypes.byref(b))
    assert f(10, 4, 1, *out) == 0
    for log_height, width, n_keys in ((10, 0, 1), (10, 33, 1), (10, 4, 0), (10, 4, 5), (29, 4, 1)):
        t.value = r.value = b.value = 7
        assert f(log_height, width, n_keys, *out) == INVALID
        assert (t.value, r.value, b.value) == (7, 7, 7)
    assert f(10, 4, 1, None, ctypes.byref(r), ctypes.byref(b)) == INVALID
    assert f(10, 4, 1, ctypes.byref(t), None, ctypes.byref(b)) == INVALID
    assert f(10, 4, 1, ctypes.byref(t), ctypes.byref(r), None) == INVALID
    with pytest.raises(Exception):
        CS.trace_sort_launch_info(10, 33, 1)


# ---- the mirror's own checks (nothing reaches the library) ------------------------------------

@pytest.mark.parametrize("keys,copies,perm,width", [
    ([0], [], None, 4),                                        # no output
    ([], [(0, 1)], None, 4),                                   # no key
    ([0, 1, 2, 3, 4], [(0, 5)], None, 8),                      # 5 keys
    ([0], [(0, 1 + c) for c in range(17)], None, 32),          # 17 copies
    ([0, 1], [(2, 1)], None, 4),                               # a destination that is a key
    ([0], [(1, 2), (2, 3)], None, 4),                          # ... a source
    ([0], [(0, 2), (1, 2)], None, 4),                          # ... another destination
    ([0], [(0, 2)], 2, 4),                                     # ... the perm column
    ([0], [(0, 1)], 0, 4),                                     # the perm column is a key
    ([0], [(1, 2)], 1, 4),                                     # the perm column is a source
    ([4], [(0, 1)], None, 4),                                  # a key at width
    ([0], [(4, 1)], None, 4),                                  # a source at width
    ([0], [(0, 4)], None, 4),                                  # a destination at width
    ([0], [(0, 1)], 4, 4),                                     # the perm column at width
    ([-1], [(0, 1)], None, 4),
])
def test_sort_arrays_rejects(keys, copies, perm, width):
    with pytest.raises(ValueError):
        CS._sort_arrays(keys, copies, perm, width)


def test_sort_arrays_accepts_key_sources_and_repeated_sources():
    got = CS._sort_arrays([1, 0], [(1, 2), (0, 3), (1, 4)], 5, 6)
    assert got == ([1, 0], [1, 0, 1], [2, 3, 4], 5)
    assert CS._sort_arrays([0], [], 1, 2) == ([0], [], [], 1)
    assert CS._sort_arrays([0, 0], [(0, 1)], None, 2) == ([0, 0], [0], [1], CS.SORT_NO_COLUMN)
    assert len(CS._sort_arrays([0], [(0, 1 + c) for c in range(16)], None, 17)[2]) == 16


# ---- the model against cases written out by hand --------------------------------------------

def test_model_ties_are_stable():
    # columns (key, payload, sorted payload, pi)
    m = [5, 10, 0, 0,
         3, 11, 0, 0,
         5, 12, 0, 0,
         3, 13, 0, 0,
         5, 14, 0, 0,
         1, 15, 0, 0,
         3, 16, 0, 0,
         5, 17, 0, 0]
    out, pi = SR.sort_matrix(m, 4, [0], [(1, 2)], 3)
    assert pi == [5, 1, 3, 6, 0, 2, 4, 7]
    assert out[2::4] == [15, 11, 13, 16, 10, 12, 14, 17] and out[3::4] == pi
    assert out[0::4] == m[0::4] and out[1::4] == m[1::4]  # the key and the source stay


def test_model_two_keys_with_the_first_tied():
    # (addr, time, sorted addr, sorted time)
    m = [7, 3, 9, 9,
         2, 8, 9, 9,
         7, 1, 9, 9,
         2, 8, 9, 9,
         7, 2, 9, 9,
         2, 0, 9, 9,
         0, 5, 9, 9,
         7, 0, 9, 9]
    out, pi = SR.sort_matrix(m, 4, [0, 1], [(0, 2), (1, 3)])
    assert pi == [6, 5, 1, 3, 7, 2, 4, 0]
    assert out[2::4] == [0, 2, 2, 2, 7, 7, 7, 7] and out[3::4] == [5, 0, 8, 8, 0, 1, 2, 3]
    # the second key first: another order
    assert SR.sort_matrix(m, 4, [1, 0], [(0, 2)])[1] == [5, 7, 2, 4, 0, 6, 1, 3]


def test_model_compares_whole_unsigned_128_bit_integers():
    """A wrong limb order puts 2^32 above 2^64, a signed compare puts M - 1 or
    2^96 (top limb bit clear, but 2^127 set in M - 1) below 0."""
    vals = [2 ** 64, 1, M - 1, 2 ** 32, 0, 2 ** 96, 2 ** 127, 2 ** 31, 2 ** 63, 2 ** 95]
    m = []
    for v in vals:
        m += [v, 0]
    out, pi = SR.sort_matrix(m, 2, [0], [(0, 1)])
    assert out[1::2] == [0, 1, 2 ** 31, 2 ** 32, 2 ** 63, 2 ** 64, 2 ** 95, 2 ** 96, 2 ** 127, M - 1]
    assert pi == [4, 1, 7, 3, 8, 0, 9, 5, 6, 2]


def test_model_perm_only_and_a_repeated_source():
    m = [3, 0, 0, 1, 0, 0, 2, 0, 0, 1, 0, 0]
    out, pi = SR.sort_matrix(m, 3, [0], [], 2)
    assert pi == [1, 3, 2, 0] and out == [3, 0, 1, 1, 0, 3, 2, 0, 2, 1, 0, 0]
    out, _ = SR.sort_matrix(m, 3, [0], [(0, 1), (0, 2)])
    assert out == [3, 1, 1, 1, 1, 1, 2, 2, 2, 1, 3, 3]
    # one row
    assert SR.sort_matrix([9, 4], 2, [0], [(0, 1)]) == ([9, 9], [0])
