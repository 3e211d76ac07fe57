"""Host side of the phase-2 fill (no GPU): fill-program validation
(mlh_fill_program_create), the host interpreter mlh_fill_program_evaluate
against the plain-Python model tests/fill_reference.py, and the Python mirror
(inv, compile_fill).  Everything is bit-exact."""
import ctypes
import random
import struct

import pytest

import fill_reference as FR
from fill_reference import ADD, COL, CONST, INV, MUL, NEG, RAND, SUB, TEMP, wire
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS

M = FR.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]


def _create(w):
    lib = _lib.load()
    h = ctypes.c_void_p()
    buf = (ctypes.c_uint8 * max(len(w), 1)).from_buffer_copy(w or b"\0")
    st = lib.mlh_fill_program_create(buf, len(w), ctypes.byref(h))
    if st == 0:
        lib.mlh_fill_program_destroy(h)
    else:
        assert not h.value
    return st


def _patch(w, offset, value):
    return w[:offset] + bytes([value]) + w[offset + 1:]


def _hdr(w, **kw):
    f = list(struct.unpack("<7I", w[:28]))
    names = ["width", "n_randoms", "n_consts", "n_temps", "n_instr", "n_outputs", "reserved"]
    for k, v in kw.items():
        f[names.index(k)] = v
    return struct.pack("<7I", *f) + w[28:]


# ---- decoder -----------------------------------------------------------------------

# every operand kind as an output (the temp through an INV)
VALID_OUTPUTS = {
    "column": wire(3, 0, [], 0, [], [(2, COL, 0)]),
    "random": wire(3, 2, [], 0, [], [(0, RAND, 1)]),
    "const": wire(3, 0, [5], 0, [], [(1, CONST, 0)]),
    "temp": wire(3, 0, [], 1, [(INV, 0, (COL, 1), (0, 0))], [(2, TEMP, 0)]),
}


@pytest.mark.parametrize("name", sorted(VALID_OUTPUTS))
def test_valid_program_with_each_operand_kind_as_output(name):
    w = VALID_OUTPUTS[name]
    assert _create(w) == 0
    p = CS.FillProgram(w)
    row = [11, 22, 33]
    assert p.evaluate(row, [7, 8][:p.n_randoms]) == FR.fill_row(FR.parse(w), row, [7, 8])


def test_accessors():
    p = CS.FillProgram(FR.LOOKUP)
    assert (p.width, p.n_randoms, p.n_outputs, p.n_inverses, p.output_mask) == (5, 1, 2, 2, 0b11000)
    q = CS.FillProgram(FR.WIDE16)
    assert (q.width, q.n_randoms, q.n_outputs, q.n_inverses) == (32, 2, 16, 16)
    assert q.output_mask == 0xFFFF0000
    assert CS.FillProgram(FR.PRODUCT).n_inverses == 0


_ONE = [(ADD, 0, (COL, 0), (COL, 0))]
_INV_CHAIN = [(INV, i % 2, (COL, i % 3), (0, 0)) for i in range(17)]

REJECTED = {
    # what mlh_cs_program_create rejects
    "truncated_header": FR.LOOKUP[:20],
    "empty": b"",
    "trailing_byte": FR.LOOKUP + b"\0",
    "column_out_of_range": wire(3, 0, [], 1, [(ADD, 0, (COL, 3), (COL, 0))], [(2, TEMP, 0)]),
    "random_out_of_range": wire(3, 1, [], 1, [(ADD, 0, (RAND, 1), (COL, 0))], [(2, TEMP, 0)]),
    "const_out_of_range": wire(3, 0, [1], 1, [(ADD, 0, (CONST, 1), (COL, 0))], [(2, TEMP, 0)]),
    "temp_out_of_range": wire(3, 0, [], 1, _ONE, [(2, TEMP, 1)]),
    "dst_out_of_range": wire(3, 0, [], 1, [(ADD, 1, (COL, 0), (COL, 0))], [(2, COL, 0)]),
    "bad_opcode": wire(3, 0, [], 1, [(5, 0, (COL, 0), (COL, 0))], [(2, TEMP, 0)]),
    "bad_kind": wire(3, 0, [], 1, [(ADD, 0, (4, 0), (COL, 0))], [(2, TEMP, 0)]),
    "bad_output_kind": wire(3, 0, [], 0, [], [(2, 4, 0)]),
    "temp_read_before_written": wire(3, 0, [], 2, [(ADD, 0, (TEMP, 1), (COL, 0))], [(2, TEMP, 0)]),
    "output_temp_never_written": wire(3, 0, [], 1, [], [(2, TEMP, 0)]),
    "non_canonical_const": wire(3, 0, [M], 0, [], [(2, CONST, 0)]),
    "instr_reserved_byte": _patch(wire(3, 0, [], 1, _ONE, [(2, TEMP, 0)]), 28 + 6, 1),
    "output_reserved_byte": _patch(wire(3, 0, [], 0, [], [(2, COL, 0)]), 28 + 3, 1),
    "neg_with_b": wire(3, 0, [], 1, [(NEG, 0, (COL, 0), (COL, 1))], [(2, TEMP, 0)]),
    "width_zero": wire(0, 0, [], 0, [], [(0, CONST, 0)]),
    "width_above_limit": wire(33, 0, [], 0, [], [(0, COL, 0)]),
    "temps_above_limit": _hdr(wire(3, 0, [], 1, [], [(2, COL, 0)]), n_temps=33),
    "consts_above_limit": wire(3, 0, [1] * 65, 0, [], [(2, COL, 0)]),
    "randoms_above_limit": wire(3, 65, [], 0, [], [(2, COL, 0)]),
    "instructions_above_limit": wire(3, 0, [], 1, _ONE * 4097, [(2, TEMP, 0)]),
    # what only fill programs have
    "no_outputs": wire(3, 0, [], 0, [], []),
    "more_outputs_than_columns": wire(2, 0, [], 0, [], [(0, COL, 0), (1, COL, 0), (1, COL, 1)]),
    "duplicate_output_column": wire(3, 0, [], 0, [], [(1, COL, 0), (1, COL, 2)]),
    "output_column_out_of_range": wire(3, 0, [], 0, [], [(3, COL, 0)]),
    "reserved_header_word": wire(3, 0, [], 0, [], [(2, COL, 0)], reserved=1),
    "inv_with_b": wire(3, 0, [], 1, [(INV, 0, (COL, 0), (COL, 1))], [(2, TEMP, 0)]),
    "seventeen_inverses": wire(3, 0, [], 2, _INV_CHAIN, [(2, TEMP, 0)]),
    "inv_of_inv": wire(3, 0, [], 1, [(INV, 0, (COL, 0), (0, 0)), (INV, 0, (TEMP, 0), (0, 0))],
                       [(2, TEMP, 0)]),
    "inv_of_value_derived_from_inv": wire(
        3, 0, [], 2, [(INV, 0, (COL, 0), (0, 0)), (ADD, 1, (COL, 1), (TEMP, 0)),
                      (INV, 0, (TEMP, 1), (0, 0))], [(2, TEMP, 0)]),
}


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_invalid_fill_program_is_rejected(name):
    assert _create(REJECTED[name]) == INVALID


def test_limits_are_accepted_and_taint_follows_the_value():
    assert _create(wire(3, 0, [], 2, _INV_CHAIN[:16], [(2, TEMP, 0)])) == 0  # 16 INVs
    # temp 0 holds an inverse, is overwritten by an untainted value, and that feeds an INV
    assert _create(wire(3, 0, [], 2, [(INV, 0, (COL, 0), (0, 0)), (ADD, 1, (COL, 1), (TEMP, 0)),
                                      (ADD, 0, (COL, 1), (COL, 2)), (INV, 0, (TEMP, 0), (0, 0))],
                        [(2, TEMP, 0), (0, TEMP, 1)])) == 0
    # every limit at its maximum
    ins = [(ADD, i % 32, (COL, i % 32), (CONST, i % 64)) for i in range(4096)]
    big = wire(32, 64, list(range(64)), 32, ins, [(j, TEMP, j) for j in range(32)])
    assert _create(big) == 0
    assert _create(FR.WIDE16) == 0


def test_every_truncation_is_rejected():
    w = FR.LOOKUP
    assert _create(w) == 0
    for n in range(len(w)):
        assert _create(w[:n]) == INVALID, n


def test_constraint_programs_still_reject_op_4():
    lib = _lib.load()
    w = CS.encode_program(3, 0, [], 1, [(4, 0, (COL, 0), (0, 0))], [(TEMP, 0)], 1)
    h = ctypes.c_void_p()
    buf = (ctypes.c_uint8 * len(w)).from_buffer_copy(w)
    assert lib.mlh_cs_program_create(buf, len(w), ctypes.byref(h)) == INVALID
    assert not h.value


def test_null_arguments():
    lib = _lib.load()
    h = ctypes.c_void_p()
    buf = (ctypes.c_uint8 * len(FR.LOOKUP)).from_buffer_copy(FR.LOOKUP)
    assert lib.mlh_fill_program_create(None, len(FR.LOOKUP), ctypes.byref(h)) == INVALID
    assert lib.mlh_fill_program_create(buf, len(FR.LOOKUP), None) == INVALID
    p = CS.FillProgram(FR.LOOKUP)
    row, out = CS._elems([1, 2, 3, 4, 5]), (ctypes.c_uint8 * 80)()
    assert lib.mlh_fill_program_evaluate(p.h, row, None, out) == INVALID  # n_randoms = 1
    assert lib.mlh_fill_program_evaluate(p.h, None, CS._elems([9]), out) == INVALID
    assert lib.mlh_fill_program_evaluate(p.h, row, CS._elems([9]), None) == INVALID
    assert lib.mlh_fill_program_evaluate(p.h, CS._elems([1, 2, 3, 4, M]), CS._elems([9]), out) == INVALID
    assert lib.mlh_fill_program_evaluate(p.h, row, CS._elems([9]), out) == 0
    t, k, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    f = lib.mlh_trace_fill_launch_info
    assert f(None, 3, ctypes.byref(t), ctypes.byref(k), ctypes.byref(b)) == INVALID
    assert f(p.h, 33, ctypes.byref(t), ctypes.byref(k), ctypes.byref(b)) == INVALID
    assert f(p.h, 3, None, ctypes.byref(k), ctypes.byref(b)) == INVALID


# ---- host interpreter against the model ------------------------------------------------

PROGRAMS = {"lookup": FR.LOOKUP, "product": FR.PRODUCT, "self": FR.SELF, "wide16": FR.WIDE16,
            "zeros": FR.ZEROS}


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_host_interpreter_matches_model(name):
    w = PROGRAMS[name]
    p = CS.FillProgram(w)
    model = FR.parse(w)
    r = random.Random(name)
    for trial in range(12):
        row = [r.randrange(M) for _ in range(p.width)]
        rnd = [r.randrange(M) for _ in range(p.n_randoms)]
        if trial % 3 == 0:
            row[0] = 0
        if trial == 1 and p.n_randoms:
            row[0] = rnd[0]  # the lookup's denominator is zero
        want = FR.fill_row(model, row, rnd)
        got = p.evaluate(row, rnd)
        assert got == want
        for j in range(p.width):  # the other columns are the input's
            if not (p.output_mask >> j) & 1:
                assert got[j] == row[j]
    if name == "zeros":
        assert p.evaluate([0, 5, 6], [9]) == [0, 0, 9]
    if name == "self":
        assert p.evaluate([3, 4], [10]) == [3, 22]
    if name == "lookup":
        g, a = 1000, 1000
        assert p.evaluate([a, 1, 2, 7, 7], [g])[3] == 0


def test_launch_info_follows_the_documented_rule():
    """B = the largest of 256 / 128 / 64 whose (width + temps + inverses) slots
    fit 152 KiB; K = the largest power of two up to 16 that leaves 512 chunks,
    1 without an INV."""
    for w, slots in ((FR.LOOKUP, 10), (FR.INV2, 4), (FR.WIDE16, 66), (FR.PRODUCT, 4)):
        p = CS.FillProgram(w)
        for L in (0, 5, 12, 17, 18, 20, 21, 22, 26, 32):
            B, K, blocks = p.launch_info(L)
            assert B in (64, 128, 256) and slots * 16 * B <= 152 * 1024
            assert B == 256 or slots * 16 * 2 * B > 152 * 1024
            assert K in (1, 2, 4, 8, 16) and (p.n_inverses or K == 1)
            chunks = -(-(1 << L) // (B * K))
            assert K == 1 or chunks >= 512
            assert K == 16 or not p.n_inverses or -(-(1 << L) // (B * 2 * K)) < 512
            assert 1 <= blocks <= min(chunks, 512)
            assert blocks * p.n_inverses * (K - 1) * B * 16 <= 64 << 20  # the prefix scratch
    assert CS.FillProgram(FR.LOOKUP).launch_info(20) == (256, 8, 512)
    assert CS.FillProgram(FR.LOOKUP).launch_info(0) == (256, 1, 1)


# ---- Python mirror ---------------------------------------------------------------------

def _lookup_assignments():
    return {3: CS.inv(CS.rand(0) - CS.var(0)), 4: -CS.var(2) * CS.inv(CS.rand(0) - CS.var(1))}


def test_compile_fill_lookup_bytes_are_pinned():
    w = CS.compile_fill(_lookup_assignments(), 5, 1)
    assert w.hex() == (
        "05000000" "01000000" "00000000" "03000000" "06000000" "02000000" "00000000"
        "0100010000000000"   # t0 = rand0 - col0
        "0400030000000000"   # t0 = inv(t0)
        "0301000200000000"   # t1 = -col2
        "0102010000010000"   # t2 = rand0 - col1
        "0402030200000000"   # t2 = inv(t2)
        "0202030103020000"   # t2 = t1 * t2
        "03030000" "04030200")
    assert w == FR.LOOKUP
    assert _create(w) == 0
    # ascending column order whatever the dict's order
    rev = dict(reversed(list(_lookup_assignments().items())))
    p = CS.FillProgram(CS.compile_fill(rev, 5, 1))
    assert p.output_mask == 0b11000
    row = [5, 6, 7, 0, 0]
    assert p.evaluate(row, [100]) == FR.fill_row(FR.parse(FR.LOOKUP), row, [100])


def test_compile_fill_errors():
    x = CS.var(0)
    with pytest.raises(ValueError):
        CS.compile_fill({1: CS.inv(CS.inv(x))}, 2, 0)
    with pytest.raises(ValueError):
        CS.compile_fill({1: CS.inv(x + CS.inv(x) * 3)}, 2, 0)
    e16 = sum((CS.inv(x + i) for i in range(1, 16)), CS.inv(x))
    assert _create(CS.compile_fill({1: e16}, 2, 0)) == 0
    with pytest.raises(ValueError):
        CS.compile_fill({1: e16 + CS.inv(x + 16)}, 2, 0)
    with pytest.raises(ValueError):
        CS.compile_fill({2: x}, 2, 0)  # column outside the trace


def test_compile_program_rejects_inv():
    with pytest.raises(ValueError):
        CS.compile_program([CS.var(0) * CS.inv(CS.var(1)) - 1], 2, 0, 2)
