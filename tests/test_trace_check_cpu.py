"""The witness check without a GPU: the plain-Python model
(tests/check_reference.py) on hand-counted cases, the argument errors the
Python mirror raises before it reaches the library, and the new symbols in the
header, the library and the ctypes table."""
import ctypes
import os
import re

import pytest
import torch

import check_reference as CR
import public_reference as PUB
import shifted_reference as SR
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS

M = CR.M
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mlh_trace_check", "mlh_trace_check_launch_info", "mlh_trace_check_shaped",
           "mlh_trace_check_public"]


# ---- the model on hand-counted cases ---------------------------------------------------------

def test_model_hand_counted_four_rows():
    """Columns (x, y): constraint 0 is x, constraint 1 is y.  Row 2 breaks both,
    row 3 breaks constraint 0 only."""
    fns = [lambda v, r: v[0], lambda v, r: v[1]]
    matrix = [0, 0,
              0, 0,
              5, 7,
              M - 1, 0]
    assert CR.check(fns, matrix, 2, [], 2) == (2, 2, 0, [2, 1], [2, 2])


def test_model_clean_and_single_row():
    fns = [lambda v, r: v[0] - v[1], lambda v, r: (v[0] + r[0]) % M]
    assert CR.check(fns, [3, 3, 4, 4], 2, [], 1, [0]) == (2, 0, 1, [0, 2], [None, 0])
    assert CR.check(fns[:1], [3, 3, 4, 4], 2, [], 1, [0]) == (0, None, None, [0], [None])
    # one row is its own next row: next(x) - x holds whatever x is
    assert CR.check([lambda v, r: v[1] - v[0]], [9], 1, [0], 0) == (0, None, None, [0], [None])


def test_model_next_row_wraps_and_zero_is_mod_m():
    """next(x) = x + 1 on the counter 0, 1, 2, 3: only the wrap 3 -> 0 breaks; a
    value that is a multiple of M counts as zero."""
    step = [lambda v, r: v[1] - v[0] - 1]
    assert CR.check(step, [0, 1, 2, 3], 1, [0], 2) == (1, 3, 0, [1], [3])
    assert CR.check([lambda v, r: v[0] + v[1]], [M - 1, 1, 2 ** 100, M - 2 ** 100], 2, [], 1) == (
        0, None, None, [0], [None])


def test_model_fibonacci_breaks_where_the_trace_says():
    assert CR.check(SR.FIB_FNS, SR.fib_matrix(4), 3, [0, 1], 4)[0] == 0
    assert CR.check(SR.FIB_FNS, SR.fib_matrix(4, ungated_wrap=True), 3, [0, 1], 4) == (
        1, 15, 0, [1, 1], [15, 15])
    # the restart at row 7 breaks the step 6 -> 7 and nothing else
    assert CR.check(SR.FIB_FNS, SR.fib_matrix(4, restart_at=7), 3, [0, 1], 4) == (
        1, 6, 0, [1, 1], [6, 6])


def test_model_public_strip():
    descs = [("first",), ("row",), ("sparse", {1: 9})]
    H, W = 4, 4
    good = PUB.with_strip([11, 12, 13, 14], 1, descs, H)
    assert CR.check_public(good, W, descs, 2) == (0, None, None, [0, 0, 0], [None, None, None])
    bad = list(good)
    bad[0] = 99              # a committed column: not looked at
    bad[2 * W + 3] = 1       # a nonzero cell where the sparse column has no entry
    bad[3 * W + 1] = 1       # a second 1 in the FIRST column
    bad[3 * W + 2] = 2       # the row index of another row
    assert CR.check_public(bad, W, descs, 2) == (2, 2, 2, [1, 1, 1], [3, 3, 2])


# ---- the mirror's argument errors ----------------------------------------------------------------

def _fib_program():
    wire, shifts = SR.program("fib4")
    return CS.Program(wire), shifts


def test_mirror_rejects_before_the_library():
    prog, shifts = _fib_program()
    assert (prog.width, shifts) == (5, [0, 1])
    t3 = CS.Trace(torch.zeros((3 * 4, 4), dtype=torch.int32), 3)  # (host memory: never reached)
    t4 = CS.Trace(torch.zeros((4 * 4, 4), dtype=torch.int32), 4)
    with pytest.raises(ValueError, match="columns wide"):  # width mismatch
        t4.check(prog, (), shifts)
    with pytest.raises(ValueError, match="outside the trace"):  # source column at the width
        t3.check(prog, (), [0, 3])
    with pytest.raises(ValueError, match="outside the trace"):
        t3.check(prog, (), [-1, 0])
    with pytest.raises(ValueError, match="columns wide"):  # W + K other than the program's width
        t3.check(prog, (), [0])
    with pytest.raises(ValueError, match="columns wide"):
        t3.check(prog, (), [0, 1, 1])
    with pytest.raises(ValueError, match="randoms"):
        t3.check(prog, (5,), shifts)


def test_check_result_fields():
    r = CS.CheckResult(2, 2, 0, [2, 1], [2, 2 ** 64 - 1])
    assert (r.bad_rows, r.first_bad_row, r.first_bad_constraint, r.ok) == (2, 2, 0, False)
    assert r.counts == [2, 1] and r.first_rows == [2, None]
    clean = CS.CheckResult(0, 2 ** 64 - 1, 2 ** 32 - 1, [0], [2 ** 64 - 1])
    assert clean.ok and clean.first_bad_row is None and clean.first_bad_constraint is None
    assert CR.as_tuple(clean) == (0, None, None, [0], [None])


# ---- the symbols ---------------------------------------------------------------------------------------

def test_symbols_in_header_library_and_table():
    src = open(os.path.join(ROOT, "include", "mlhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert "mlh_trace_check_report" in code
    assert ctypes.sizeof(_lib.TraceCheckReportC) == 24
    # the header cites the reference where it gives the semantics
    assert "constraints.rs:3-10" in src and "evaluation.rs:21-29" in src


def test_launch_info_needs_no_gpu():
    prog, _ = _fib_program()
    threads, blocks = CS.trace_check_launch_info(prog, 0)
    assert (threads, blocks) == (256, 1)
    assert CS.trace_check_launch_info(prog, 12) == (256, 4)
    assert CS.trace_check_launch_info(prog, 32) == (256, 1024)
    with pytest.raises(_lib.MlhError):
        CS.trace_check_launch_info(prog, 33)
    t, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib_status(None, 4, t, b) == _lib.STATUS_CODES["MLH_ERR_INVALID"]


def lib_status(prog, log_height, t, b):
    return _lib.load().mlh_trace_check_launch_info(prog, log_height, ctypes.byref(t), ctypes.byref(b))
