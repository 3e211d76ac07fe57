"""mlh_trace_check and mlh_trace_check_public on the GPU against the
plain-Python model tests/check_reference.py: the default launch and the shapes
of mlh_trace_check_shaped where the seams are (a chunk's last lane, whose next
row comes from global memory; the chunks of several blocks; the cyclic wrap),
the field's zero, the width and count limits, seeded random programs, purity,
the argument errors, the public strip kind by kind, the stream promise, scratch
poison, and a PhasedProver end to end.  Every comparison is exact."""
import ctypes
import functools
import random

import pytest

import check_reference as CR
import program_fuzz as PF
import public_reference as PUB
import shifted_reference as SR
import stream_harness as H
import test_stream_contract_gpu as TSC
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.transcript import Transcript

pytestmark = pytest.mark.gpu

M = CR.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]

# (threads, max blocks) of mlh_trace_check_shaped; None: mlh_trace_check
SHAPES = [(64, 1),      # every chunk in one block: the per-block widening, the seam per chunk
          (64, 3),      # chunks dealt to three blocks, unevenly
          (128, 2),
          (256, 1024),
          None]


# ---- helpers ---------------------------------------------------------------------------------------

def _dev(vals):
    return D.to_device(D.ints_to_limbs(vals))


def _check(dev, W, prog, shifts=(), randoms=(), shape=None):
    return CR.as_tuple(CS.Trace(dev, W).check(prog, randoms, shifts, shape=shape))


def _all_shapes(vals, W, prog, shifts, randoms, want, shapes=SHAPES):
    """The model's tuple under every shape, and the matrix untouched."""
    dev = _dev(vals)
    before = D.from_device(dev).tobytes()
    for shape in shapes:
        assert _check(dev, W, prog, shifts, randoms, shape) == want, shape
    assert D.from_device(dev).tobytes() == before


@functools.lru_cache(maxsize=None)
def _system(name):
    """-> (Program, shift list, fns, W, randoms) of a system of shifted_reference."""
    wire, shifts = SR.program(name)
    _, fns, _, W, n_rand = SR._system(name)[:5]
    return CS.Program(wire), shifts, fns, W, PF.elements("check " + name, n_rand)


def _matrix(name, L, seed=0):
    W = _system(name)[3]
    return SR.fib_matrix(L) if name.startswith("fib") else PF.matrix("check %s %d" % (name, seed), 1 << L, W)


# ---- heights and shapes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fib4", "mixed5"])
@pytest.mark.parametrize("L", [0, 1])
def test_one_and_two_rows(name, L):
    """L = 0: the row is its own next row."""
    prog, shifts, fns, W, rnd = _system(name)
    for vals in (_matrix(name, L), PF.matrix("tiny %s" % name, 1 << L, W)):
        want = CR.check(fns, vals, W, shifts, L, rnd)
        _all_shapes(vals, W, prog, shifts, rnd, want, [None, (64, 1), (256, 1024)])


@pytest.mark.parametrize("L", [6, 9, 12])
def test_satisfied_fibonacci(L):
    prog, shifts, fns, W, rnd = _system("fib4")
    _all_shapes(SR.fib_matrix(L), W, prog, shifts, rnd, (0, None, None, [0, 0], [None, None]))
    res = CS.Trace(_dev(SR.fib_matrix(L)), W).check(prog, (), shifts)
    assert res.ok and res.first_bad_row is None and res.first_bad_constraint is None


@pytest.mark.parametrize("L", [6, 9, 12])
def test_broken_fibonacci_names_rows_and_constraints(L):
    prog, shifts, fns, W, rnd = _system("fib4")
    Hh = 1 << L
    vals = SR.fib_matrix(L, ungated_wrap=True)
    want = CR.check(fns, vals, W, shifts, L)
    assert want == (1, Hh - 1, 0, [1, 1], [Hh - 1, Hh - 1])
    _all_shapes(vals, W, prog, shifts, rnd, want)
    for r in sorted({1, 63, min(64, Hh - 1), Hh // 2 + 1, Hh - 1}):  # the step r - 1 -> r breaks
        vals = SR.fib_matrix(L, restart_at=r)
        want = CR.check(fns, vals, W, shifts, L)
        assert want == (1, r - 1, 0, [1, 1], [r - 1, r - 1])
        _all_shapes(vals, W, prog, shifts, rnd, want)


@pytest.mark.parametrize("L", [6, 9, 12])
def test_mixed_system_on_a_random_trace(L):
    """One random, one shift, two constraints that fail almost everywhere."""
    prog, shifts, fns, W, rnd = _system("mixed5")
    vals = _matrix("mixed5", L)
    want = CR.check(fns, vals, W, shifts, L, rnd)
    assert want[0] > (1 << L) // 2
    _all_shapes(vals, W, prog, shifts, rnd, want)


def test_launch_info_is_the_default_shape():
    prog = _system("fib4")[0]
    assert CS.trace_check_launch_info(prog, 9) == (256, 1)
    assert CS.trace_check_launch_info(prog, 12) == (256, 4)
    wide = _system("wide9")[0]
    assert CS.trace_check_launch_info(wide, 22)[0] == 256  # 32 columns and one temp


# ---- the seams ----------------------------------------------------------------------------------------------

# next(a) = a + d, cyclically: a cell of d breaks exactly its own row, a cell of a its row and the one before
def _running_sum_system():
    wire, shifts = CS.compile_shifted([CS.nxt(0) - CS.var(0) - CS.var(1)], 2, 0, 1)
    return CS.Program(wire), shifts, [lambda v, r: (v[2] - v[0] - v[1]) % M]


@functools.lru_cache(maxsize=None)
def _running_sum_matrix(L):
    r = random.Random(515)
    Hh = 1 << L
    a = [r.randrange(M) for _ in range(Hh)]
    return [x for i in range(Hh) for x in (a[i], (a[(i + 1) % Hh] - a[i]) % M)]


SEAM_L = 9
SEAM_ROWS = {"row 0": 0, "a chunk's last lane": 63, "the next chunk's first": 64,
             "the last row of block 2 of 3": 6 * 64 - 1, "the last row of block 0 of 3": 7 * 64 - 1,
             "the last row": (1 << SEAM_L) - 1}


@pytest.mark.parametrize("where", sorted(SEAM_ROWS))
def test_one_bad_cell_at_a_seam(where):
    prog, shifts, fns = _running_sum_system()
    row = SEAM_ROWS[where]
    vals = list(_running_sum_matrix(SEAM_L))
    assert CR.check(fns, vals, 2, shifts, SEAM_L)[0] == 0
    vals[2 * row + 1] = (vals[2 * row + 1] + 1) % M
    want = CR.check(fns, vals, 2, shifts, SEAM_L)
    assert want == (1, row, 0, [1], [row])
    _all_shapes(vals, 2, prog, shifts, (), want, [(64, 1), (64, 3), (64, 1024), None])


def test_row_zero_source_breaks_the_last_row():
    """Only row 0's source column changes: the last row's next row is row 0."""
    prog, shifts, fns = _running_sum_system()
    vals = list(_running_sum_matrix(SEAM_L))
    vals[0] = (vals[0] + 1) % M
    want = CR.check(fns, vals, 2, shifts, SEAM_L)
    last = (1 << SEAM_L) - 1
    assert want == (2, 0, 0, [2], [0])
    _all_shapes(vals, 2, prog, shifts, (), want, [(64, 1), (64, 3), (128, 2), None])
    # with row 0 repaired through its own d, only the wrap is left
    vals[1] = (vals[1] - 1) % M
    want = CR.check(fns, vals, 2, shifts, SEAM_L)
    assert want == (1, last, 0, [1], [last])
    _all_shapes(vals, 2, prog, shifts, (), want, [(64, 1), (64, 3), (128, 2), None])


# ---- zero is the field's zero ------------------------------------------------------------------------------------

def test_sums_and_differences_that_are_zero_mod_m():
    L = 7
    r = random.Random(96)
    xs = [1, M - 1, 2 ** 96, 2 ** 96 + 5, M - 2 ** 96, 2 ** 127, M - 2] + [
        r.randrange(2 ** 96, M) for _ in range((1 << L) - 7)]
    vals = [v for x in xs for v in (x, M - x)]
    assert vals[:4] == [1, M - 1, M - 1, 1]
    prog = CS.Program(CS.compile_program([CS.var(0) + CS.var(1), CS.var(0) - CS.var(0)], 2, 0, 1))
    fns = [lambda v, r: v[0] + v[1], lambda v, r: v[0] - v[0]]
    want = CR.check(fns, vals, 2, [], L)
    assert want == (0, None, None, [0, 0], [None, None])
    _all_shapes(vals, 2, prog, [], (), want)
    vals[2 * 77 + 1] = (vals[2 * 77 + 1] + 1) % M  # off by one: the sum is 1
    _all_shapes(vals, 2, prog, [], (), (1, 77, 0, [1, 0], [77, None]))


def test_constant_one_fails_on_every_row():
    """4096 rows in 64 chunks of one block: the 32-bit chunk counts widen into
    the block's 64-bit total."""
    L, Hh = 12, 1 << 12
    prog = CS.Program(CS.compile_program([CS.const(1), CS.var(0) - CS.var(0)], 1, 0, 1))
    vals = PF.matrix("const one", Hh, 1)
    _all_shapes(vals, 1, prog, [], (), (Hh, 0, 0, [Hh, 0], [0, None]))


# ---- width and count limits ----------------------------------------------------------------------------------------

def test_thirty_two_columns():
    """W = 16 and K = 16 in descending order: the wide system."""
    prog, shifts, fns, W, rnd = _system("wide9")
    L = 7
    vals = PF.matrix("wide", 1 << L, W)
    for i in (3, 63, 64, 127):  # all zero: the one constraint holds there
        vals[i * W:(i + 1) * W] = [0] * W
    want = CR.check(fns, vals, W, shifts, L)
    assert 0 < want[3][0] < (1 << L) - 4  # those rows, and rows whose next row is one of them
    _all_shapes(vals, W, prog, shifts, rnd, want)


def _many_constraints():
    """256 constraints over 32 temps and 32 constants (the wire format holds no
    more of either): temp t = var(t mod W) - const(t + 1), constraint c = temp
    c mod 32.  A cell of column j that holds t + 1, t mod W == j, satisfies the
    8 constraints of temp t and no other of that column."""
    W, T = 8, 32
    consts = [t + 1 for t in range(T)]
    instrs = [(CS.OP_SUB, t, (CS.COL, t % W), (CS.CONST, t)) for t in range(T)]
    outs = [(CS.TEMP, c % T) for c in range(256)]
    fns = [(lambda v, r, c=c: v[(c % T) % W] - consts[c % T]) for c in range(256)]
    return CS.Program(CS.encode_program(W, 0, consts, T, instrs, outs, 1)), fns, W


def test_256_constraints_known_subset():
    prog, fns, W = _many_constraints()
    assert prog.n_constraints == 256
    L, Hh = 7, 1 << 7
    r = random.Random(256)
    vals = []
    for i in range(Hh):  # column j holds j + 1 + 8 q (temp j + 8 q is zero) or, q == 4, something else
        vals += [j + 1 + 8 * q if q < 4 else 1000 + i for j in range(W) for q in [r.randrange(5)]]
    want = CR.check(fns, vals, W, [], L)
    assert want[0] == Hh and 0 < min(want[3]) and max(want[3]) < Hh  # every constraint: some rows, not all
    assert [want[3][c] for c in range(32)] == [want[3][c + 32 * k] for c in range(32) for k in [3]]
    assert CS.trace_check_launch_info(prog, L)[0] == 128  # 40 slots: 256 threads do not fit
    _all_shapes(vals, W, prog, [], (), want, [(64, 1), (64, 3), (128, 1024), None])
    # a trace that satisfies constraints c with c mod 32 < 8 everywhere
    vals = [j + 1 for _ in range(Hh) for j in range(W)]
    want = CR.check(fns, vals, W, [], L)
    assert [n == 0 for n in want[3]] == [c % 32 < 8 for c in range(256)]
    assert want[:3] == (Hh, 0, 8)
    _all_shapes(vals, W, prog, [], (), want, [(64, 3), None])


# ---- random programs -----------------------------------------------------------------------------------------------

FUZZ_L = 7  # two chunks of 64 rows
FUZZ = [("expr", s) for s in (1, 2, 3, 4, 5, 6, 7, 8)] + [("instr", s) for s in (1, 2, 3, 4, 5, 6)]


def _make_hold(case, vals, rnd):
    """Rewrite one column so that one constraint holds on every row: the first
    (constraint, column) for which the constraint, taken as affine in the
    column's cell, has a root on every row that the closure confirms.  ->
    (the constraint or None, the matrix)."""
    W, rows = case.width, len(vals) // case.width
    for c, f in enumerate(case.fns):
        for j in range(W):
            out, ok = list(vals), True
            for i in range(rows):
                row = out[i * W:(i + 1) * W]
                row[j] = 0
                v0 = f(row, rnd) % M
                row[j] = 1
                slope = (f(row, rnd) - v0) % M
                if slope == 0:
                    ok = False
                    break
                row[j] = -v0 * pow(slope, M - 2, M) % M
                if f(row, rnd) % M != 0:
                    ok = False
                    break
                out[i * W + j] = row[j]
            if ok:
                return c, out
    return None, vals


@functools.lru_cache(maxsize=None)
def _fuzz_case(kind, seed):
    """-> (Program, shifts, fns, W, randoms, matrix, model result, the constraint made to hold)."""
    if kind == "expr":
        case = PF.expr_case(seed, nxt=True, width=None if seed % 2 else 5)
        shifts = list(case.got_shifts)
        assert shifts == list(case.shifts)
    else:
        case = PF.instr_case(seed, width=None if seed % 2 else 4)
        shifts = []
    W = case.width
    rnd = PF.elements("check fuzz %s %d" % (kind, seed), case.n_randoms)
    vals = PF.matrix("check fuzz %s %d" % (kind, seed), 1 << FUZZ_L, W)
    held = None
    if not shifts:  # (a next-row operand would couple the rows)
        held, vals = _make_hold(case, vals, rnd)
    want = CR.check(case.fns, vals, W, shifts, FUZZ_L, rnd)
    return CS.Program(case.wire), shifts, case.fns, W, rnd, vals, want, held


@pytest.mark.parametrize("kind,seed", FUZZ)
def test_random_program_against_the_plain_evaluator(kind, seed):
    prog, shifts, fns, W, rnd, vals, want, held = _fuzz_case(kind, seed)
    assert prog.width == W + len(shifts) and prog.n_constraints == len(fns)
    if held is not None:
        assert want[3][held] == 0
    _all_shapes(vals, W, prog, shifts, rnd, want, [(64, 1), (64, 3), None])


def test_random_programs_cover_both_outcomes():
    assert len(FUZZ) >= 12
    counts = [n for kind, seed in FUZZ for n in _fuzz_case(kind, seed)[6][3]]
    assert any(n == 0 for n in counts) and any(n > 0 for n in counts)
    assert any(_fuzz_case(kind, seed)[7] is not None for kind, seed in FUZZ)
    assert any(_fuzz_case(kind, seed)[1] for kind, seed in FUZZ)  # a case with next-row operands


# ---- purity ------------------------------------------------------------------------------------------------------------

def _raw(dev, L, W, prog, shifts, rnd, shape):
    """The counters as bytes, through the C ABI."""
    n, K = prog.n_constraints, len(shifts)
    counts, firsts = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
    rep = _lib.TraceCheckReportC()
    args = (prog.h, D.ptr(dev), L, W, (ctypes.c_uint32 * max(K, 1))(*shifts), K, CS._elems(rnd),
            counts, firsts, ctypes.byref(rep))
    lib, ctx = D.lib(), D.context()
    if shape is None:
        D.check(lib.mlh_trace_check(ctx, *args), ctx)
    else:
        D.check(lib.mlh_trace_check_shaped(ctx, *args, *shape), ctx)
    return bytes(counts) + bytes(firsts) + bytes(rep)


def test_same_bytes_under_every_shape():
    prog, shifts, fns, W, rnd = _system("mixed5")
    L = 12
    vals = _matrix("mixed5", L, seed=1)
    for i in range(0, 1 << L, 5):  # rows on which both constraints hold: all zero, and the next row's column 2
        vals[i * W:(i + 1) * W] = [0] * W
        vals[((i + 1) % (1 << L)) * W + 2] = 0
    dev = _dev(vals)
    before = D.from_device(dev).tobytes()
    got = {_raw(dev, L, W, prog, shifts, rnd, shape) for shape in SHAPES + [(64, 1024), (128, 1024)]}
    assert len(got) == 1
    assert D.from_device(dev).tobytes() == before
    want = CR.check(fns, vals, W, shifts, L, rnd)
    assert 0 < want[3][0] < (1 << L)
    assert _check(dev, W, prog, shifts, rnd) == want


# ---- argument errors -------------------------------------------------------------------------------------------------------

_OK = dict(L=6, W=3, shifts=[0, 1], n_shifts=2, randoms=None, shape=None, prog=True, matrix=True,
           report=True)
BAD = {
    "width 0": dict(W=0), "width 33": dict(W=33), "width 4": dict(W=4), "width 2": dict(W=2),
    "log_height 33": dict(L=33), "one shift": dict(n_shifts=1), "three shifts": dict(n_shifts=3, shifts=[0, 1, 1]),
    "source at width": dict(shifts=[0, 3]), "null shifts": dict(shifts=None),
    "null program": dict(prog=None), "null matrix": dict(matrix=None), "null report": dict(report=None),
    "threads 32": dict(shape=(32, 8)), "threads 96": dict(shape=(96, 8)), "threads 512": dict(shape=(512, 8)),
    "no block": dict(shape=(64, 0)), "1025 blocks": dict(shape=(64, 1025)),
}


def _call_raw(a, dev, prog, counts, firsts, rep, ctx):
    lib = D.lib()
    shifts = None if a["shifts"] is None else (ctypes.c_uint32 * len(a["shifts"]))(*a["shifts"])
    args = (prog.h if a["prog"] else None, D.ptr(dev) if a["matrix"] else None, a["L"], a["W"], shifts,
            a["n_shifts"], a["randoms"], counts, firsts, ctypes.byref(rep) if a["report"] else None)
    if a["shape"] is None:
        return lib.mlh_trace_check(ctx, *args)
    return lib.mlh_trace_check_shaped(ctx, *args, *a["shape"])


@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_errors_leave_the_outputs_alone(what):
    prog = _system("fib4")[0]
    a = dict(_OK, **BAD[what])
    dev = _dev(SR.fib_matrix(6) + [0] * (40 << 6))  # room for the widest case that could be taken as valid
    counts, firsts = (ctypes.c_uint64 * 2)(7, 7), (ctypes.c_uint64 * 2)(9, 9)
    rep = _lib.TraceCheckReportC(1, 2, 3, 4)
    ctx = D.context()
    assert _call_raw(a, dev, prog, counts, firsts, rep, ctx) == INVALID, what
    assert D.lib().mlh_last_error(ctx)
    assert list(counts) == [7, 7] and list(firsts) == [9, 9]
    assert (rep.n_bad_rows, rep.first_bad_row, rep.first_bad_constraint, rep.reserved) == (1, 2, 3, 4)
    assert _call_raw(a, dev, prog, counts, firsts, rep, None) == INVALID


def test_randoms_missing_or_not_canonical_and_slots_beyond_lds():
    prog, shifts, fns, W, rnd = _system("mixed5")
    dev = _dev(_matrix("mixed5", 6))
    counts, firsts = (ctypes.c_uint64 * 2)(7, 7), (ctypes.c_uint64 * 2)(9, 9)
    rep = _lib.TraceCheckReportC(1, 2, 3, 4)
    ctx = D.context()
    base = dict(_OK, W=W, shifts=shifts, n_shifts=len(shifts))
    for bad in (None, CS._elems([M]), CS._elems([2 ** 128 - 1])):
        assert _call_raw(dict(base, randoms=bad), dev, prog, counts, firsts, rep, ctx) == INVALID
    assert list(counts) == [7, 7] and rep.reserved == 4
    assert _call_raw(dict(base, randoms=CS._elems(rnd)), dev, prog, counts, firsts, rep, ctx) == 0
    assert rep.reserved == 0
    # 32 columns and 32 temps: 64 slots fit 152 KiB at 128 threads and below, not at 256
    T = 32
    instrs = [(CS.OP_ADD, t, (CS.COL, t), (CS.COL, 31 - t)) for t in range(T)]
    big = CS.Program(CS.encode_program(32, 0, [], T, instrs, [(CS.TEMP, 0)], 1))
    assert CS.trace_check_launch_info(big, 10) == (128, 2)
    vals = PF.matrix("big", 64, 32)
    t = CS.Trace(_dev(vals), 32)
    want = CR.check([lambda v, r: v[0] + v[31]], vals, 32, [], 6)
    assert CR.as_tuple(t.check(big)) == want == CR.as_tuple(t.check(big, shape=(128, 4)))
    with pytest.raises(_lib.MlhError):
        t.check(big, shape=(256, 4))


# ---- the public strip ----------------------------------------------------------------------------------------------------------

def _six_kinds(L):
    Hh = 1 << L
    v = PF.elements("six kinds", 16)
    per = v[1:3] if L else v[1:2]
    sparse = {0: v[5]} if L == 0 else {1: v[5], Hh // 2: v[6], Hh - 1: v[7]}
    return [("const", v[0]), ("first",), ("last",), ("row",), ("periodic", per), ("sparse", sparse)]


def _public(dev, W, spec):
    return CR.as_tuple(CS.Trace(dev, W).check_public(spec))


@pytest.mark.parametrize("L", [0, 4, 9])
def test_filled_strip_is_clean_and_each_kind_is_caught(L):
    descs, Hh, W, C = _six_kinds(L), 1 << L, 8, 2
    F = len(descs)
    spec = PUB.builder(descs)
    committed = PF.matrix("strip %d" % L, Hh, C)
    t = CS.Trace(_dev([v for i in range(Hh) for v in committed[i * C:(i + 1) * C] + [3] * F]), W)
    t.fill_public(spec)
    good = D.limbs_to_ints(D.from_device(t.matrix()))
    assert good == PUB.with_strip(committed, C, descs, Hh)
    clean = (0, None, None, [0] * F, [None] * F)
    assert _public(t.matrix(), W, spec) == clean == CR.check_public(good, W, descs, L)
    tile = CS.public_fill_launch_info(L, W, F)[0]  # rows per tile
    sparse_rows = sorted(descs[5][1])
    no_entry = next(i for i in range(Hh) if i not in descs[5][1]) if L else None
    cells = {  # what is corrupted -> (row, column of the strip)
        "const": (Hh // 3, 0), "first at row 0": (0, 1), "last at the last row": (Hh - 1, 2),
        "row at a tile's last row": (min(tile, Hh) - 1, 3), "a periodic entry": (Hh // 2, 4),
        "a sparse entry's value": (sparse_rows[-1], 5), "no sparse entry": (no_entry, 5)}
    for what, (row, j) in sorted(cells.items()):
        if row is None:
            continue
        vals = list(good)
        vals[row * W + C + j] = (vals[row * W + C + j] + 1) % M
        want = CR.check_public(vals, W, descs, L)
        counts, firsts = [0] * F, [None] * F
        counts[j], firsts[j] = 1, row
        assert want == (1, row, j, counts, firsts), what
        dev = _dev(vals)
        assert _public(dev, W, spec) == want, what
        assert D.limbs_to_ints(D.from_device(dev)) == vals
    # a committed column is not looked at; several cells, two of them in one row
    vals = list(good)
    vals[0] = (vals[0] + 1) % M
    vals[(Hh - 1) * W + 1] = (vals[(Hh - 1) * W + 1] + 1) % M
    assert _public(_dev(vals), W, spec) == clean
    for row, j in ((Hh - 1, 0), (Hh - 1, 5), (0, 3)):
        vals[row * W + C + j] ^= 1
    assert _public(_dev(vals), W, spec) == CR.check_public(vals, W, descs, L)


def test_public_check_with_many_sparse_entries_and_tiles():
    """Sixteen public columns over 2^12 rows (32 tiles of 128 rows), a sparse
    column of 1000 entries: the binary search, tiles beyond the first."""
    L, Hh, W = 12, 1 << 12, 18
    r = random.Random(1000)
    rows = sorted(r.sample(range(Hh), 1000))
    big = {i: r.randrange(1, M) for i in rows}
    descs = PUB.pwide_descs(L)[:15] + [("sparse", big)]
    F, C = len(descs), W - len(descs)
    spec = PUB.builder(descs)
    t = CS.Trace(D.to_device(D.random_limbs(W << L, 18)), W)
    t.fill_public(spec)
    clean = (0, None, None, [0] * F, [None] * F)
    assert _public(t.matrix(), W, spec) == clean
    vals = D.limbs_to_ints(D.from_device(t.matrix()))
    for row, j in ((rows[0], 15), (rows[500], 15), (rows[-1], 15), (rows[3] + 1 if rows[3] + 1 not in big else rows[3], 15),
                   (Hh - 1, 7), (127, 3), (128, 3), (Hh // 2, 8), (4000, 0)):
        vals[row * W + C + j] = (vals[row * W + C + j] + 1) % M
    want = CR.check_public(vals, W, descs, L)
    assert want[0] >= 5 and want[3][15] >= 3
    assert _public(_dev(vals), W, spec) == want


def test_public_check_argument_errors():
    descs = _six_kinds(4)
    spec = PUB.builder(descs)
    dev = _dev([0] * (8 << 4))
    lib, ctx = D.lib(), D.context()
    counts, firsts = (ctypes.c_uint64 * 6)(*[7] * 6), (ctypes.c_uint64 * 6)(*[9] * 6)
    bad, first = ctypes.c_uint64(5), ctypes.c_uint64(6)
    ok = dict(ctx=ctx, spec=spec.h, m=D.ptr(dev), L=4, W=8, bad=ctypes.byref(bad), first=ctypes.byref(first))
    cases = [dict(spec=None), dict(m=None), dict(W=0), dict(W=33), dict(W=5), dict(L=33),
             dict(L=3),  # the sparse row 15 and the last row are beyond 8 rows
             dict(bad=None), dict(first=None), dict(ctx=None)]
    for c in cases:
        a = dict(ok, **c)
        st = lib.mlh_trace_check_public(a["ctx"], a["spec"], a["m"], a["L"], a["W"], counts, firsts, a["bad"], a["first"])
        assert st == INVALID, c
    assert list(counts) == [7] * 6 and list(firsts) == [9] * 6 and (bad.value, first.value) == (5, 6)


# ---- the stream promise and scratch poison ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def S():
    return H.side_stream()


def test_check_on_a_busy_stream_with_a_late_trace(S):
    """The call synchronises: the counters of the late trace, not of what stood
    in the buffer before."""
    prog, shifts, fns, W, rnd = _system("mixed5")
    L = 11
    a = D.random_limbs(W << L, 77)
    a[5 * W:6 * W] = 0          # row 5 holds ...
    a[6 * W + 2] = 0            # ... with the next row's column 2 zero
    want = CR.check(fns, D.limbs_to_ints(a), W, shifts, L, rnd)
    assert want[3][0] == (1 << L) - 1

    def call(buf):
        return _check(buf, W, prog, shifts, rnd), D.from_device(buf).tobytes()

    TSC._same(TSC._returns(S, "trace_check (11, 4)", [a], call), (want, a.tobytes()))


def test_public_check_on_a_busy_stream_with_a_late_trace(S):
    L, W = 9, 8
    descs = _six_kinds(L)
    spec = PUB.builder(descs)
    vals = PUB.with_strip(PF.matrix("late strip", 1 << L, 2), 2, descs, 1 << L)
    vals[100 * W + 2 + 3] = 99
    want = CR.check_public(vals, W, descs, L)
    assert want[:3] == (1, 100, 3)

    def call(buf):
        return _public(buf, W, spec)

    TSC._same(TSC._returns(S, "trace_check_public (9, 8)", [D.ints_to_limbs(vals)], call), want)


def test_scratch_poison_does_not_reach_the_counters():
    """The counters come from the pool: the call zeroes them on the stream
    whatever the poison word."""
    prog, shifts, fns, W, rnd = _system("fib4")
    L = 9
    vals = SR.fib_matrix(L, restart_at=200)
    want = CR.check(fns, vals, W, shifts, L)
    descs = _six_kinds(L)
    spec = PUB.builder(descs)
    pvals = PUB.with_strip(PF.matrix("poison strip", 1 << L, 2), 2, descs, 1 << L)
    pvals[300 * 8 + 2 + 5] = 1
    pwant = CR.check_public(pvals, 8, descs, L)
    assert pwant[:3] == (1, 300, 5)
    dev, pdev = _dev(vals), _dev(pvals)
    lib, ctx = D.lib(), D.context()
    got = []
    try:
        for word in (3, 0xFFFFFFFF, 0x01234567):
            D.check(lib.mlh_set_scratch_poison(ctx, word), ctx)
            for shape in ((64, 3), None):
                got.append(_check(dev, W, prog, shifts, rnd, shape))
            got.append(_public(pdev, 8, spec))
    finally:
        D.check(lib.mlh_set_scratch_poison(ctx, 0), ctx)
    assert got == [want, want, pwant] * 3


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def _pfib(L):
    """(a | b | first, last, io): a pre-random, b a phase-2 column, three public."""
    ab, result = PUB.fib_columns(L)
    descs = PUB.pfib_descs(L, result)
    cset = CS.ConstraintSet(PUB.pfib_exprs(), 2)
    layout = CS.WitnessLayout(columns=5, randoms=0, pre_random_columns=1,
                              public_columns=PUB.builder(descs))
    vals = [v for i in range(1 << L) for v in ab[2 * i:2 * i + 2] + [7, 7, 7]]  # the strip arrives unwritten
    return cset, layout, descs, vals


def test_phased_prover_check_clean_then_proof_verifies():
    L = 6
    cset, layout, descs, vals = _pfib(L)
    trace = CS.Trace(_dev(vals), 5)
    tr = Transcript()
    tr.absorb(b"check")
    vt = tr.clone()
    prover = CS.System.phased_prover(tr, cset, layout, trace)
    entry = tr.random()
    res, pub = prover.check()
    assert res.ok and pub.ok and res.counts == [0] * 4 and pub.counts == [0] * 3
    assert res.first_bad_row is None and pub.first_bad_constraint is None
    assert tr.random() == entry  # check() touches no transcript
    proof = prover.prove(tr, 0)
    assert proof.verify(vt, cset, layout, 0, 0)
    assert vt.random() == tr.random()


def test_phased_prover_check_names_the_broken_row():
    L, row = 6, 37
    cset, layout, descs, vals = _pfib(L)
    trace = CS.Trace(_dev(vals), 5)
    tr = Transcript()
    tr.absorb(b"check")
    vt = tr.clone()
    prover = CS.System.phased_prover(tr, cset, layout, trace)
    host = D.from_device(trace.matrix()).copy()
    host[row * 5 + 1, 0] ^= 1  # b, the phase-2 column, at one row
    trace.matrix().copy_(D.to_device(host))
    res, pub = prover.check()
    want = CR.check(PUB.PFIB_FNS, D.limbs_to_ints(host), 5, prover.shift_columns, L)
    assert CR.as_tuple(res) == want
    assert (res.first_bad_row, res.first_bad_constraint) == (row - 1, 1) and not res.ok
    assert res.counts == [1, 2, 0, 0] and res.first_rows == [row, row - 1, None, None]
    assert pub.ok
    proof = prover.prove(tr, 0)  # the prover still accepts the trace ...
    assert not proof.verify(vt, cset, layout, 0, 0)  # ... and the verifier rejects
