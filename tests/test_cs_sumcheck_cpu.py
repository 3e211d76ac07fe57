"""Host side of the constraint-system sumcheck (no GPU): constraint-program
validation, mlh_system_challenges, the host interpreter and
mlh_cs_sumcheck_verify, against the plain-Python model tests/cs_reference.py.
Everything is bit-exact."""
import ctypes
import random
import struct

import pytest

import cs_cases
import cs_reference as R
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd.constraint_system import (COL, CONST, OP_ADD, OP_MUL, OP_NEG, OP_SUB, RAND, TEMP,
                                               encode_program)
from multilinear_amd.transcript import Transcript
from oracle import field as F
from oracle import transcript as OT

M = F.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]
VERIFY = _lib.STATUS_CODES["MLH_ERR_VERIFY"]


def _create(wire):
    lib = _lib.load()
    h = ctypes.c_void_p()
    buf = (ctypes.c_uint8 * max(len(wire), 1)).from_buffer_copy(wire or b"\0")
    st = lib.mlh_cs_program_create(buf, len(wire), ctypes.byref(h))
    if st == 0:
        lib.mlh_cs_program_destroy(h)
    return st


def _valid_wire():
    # t0 = x0 * x1; t1 = t0 - c0; t0 = -x2 (reuse); outputs t1, t0
    ins = [(OP_MUL, 0, (COL, 0), (COL, 1)), (OP_SUB, 1, (TEMP, 0), (CONST, 0)),
           (OP_NEG, 0, (COL, 2), (0, 0))]
    return encode_program(3, 1, [9], 2, ins, [(TEMP, 1), (TEMP, 0)], 2)


def test_valid_program_round_trips_accessors():
    p = CS.Program(_valid_wire())
    assert (p.width, p.degree, p.n_constraints, p.n_randoms) == (3, 2, 2, 1)
    assert p.evaluate([3, 4, 5], [11], [2, 7]) == (2 * (3 * 4 - 9) + 7 * (M - 5)) % M


def _hdr(wire, **kw):
    f = list(struct.unpack("<7I", wire[:28]))
    names = ["width", "n_randoms", "n_consts", "n_temps", "n_instr", "n_constraints", "degree"]
    for k, v in kw.items():
        f[names.index(k)] = v
    return struct.pack("<7I", *f) + wire[28:]


REJECTED = {
    "truncated": _valid_wire()[:-1],
    "truncated_header": _valid_wire()[:20],
    "empty": b"",
    "trailing_byte": _valid_wire() + b"\0",
    "column_out_of_range": encode_program(3, 0, [], 1, [(OP_ADD, 0, (COL, 3), (COL, 0))], [(TEMP, 0)], 1),
    "random_out_of_range": encode_program(3, 1, [], 1, [(OP_ADD, 0, (RAND, 1), (COL, 0))], [(TEMP, 0)], 1),
    "const_out_of_range": encode_program(3, 0, [1], 1, [(OP_ADD, 0, (CONST, 1), (COL, 0))], [(TEMP, 0)], 1),
    "temp_out_of_range": encode_program(3, 0, [], 1, [(OP_ADD, 0, (COL, 0), (COL, 0))], [(TEMP, 1)], 1),
    "dst_out_of_range": encode_program(3, 0, [], 1, [(OP_ADD, 1, (COL, 0), (COL, 0))], [(COL, 0)], 1),
    "bad_opcode": encode_program(3, 0, [], 1, [(4, 0, (COL, 0), (COL, 0))], [(TEMP, 0)], 1),
    "bad_kind": encode_program(3, 0, [], 1, [(OP_ADD, 0, (4, 0), (COL, 0))], [(TEMP, 0)], 1),
    "temp_read_before_written": encode_program(3, 0, [], 2, [(OP_ADD, 0, (TEMP, 1), (COL, 0))],
                                               [(TEMP, 0)], 1),
    "output_temp_never_written": encode_program(3, 0, [], 1, [], [(TEMP, 0)], 1),
    "non_canonical_const": encode_program(3, 0, [M], 1, [(OP_ADD, 0, (CONST, 0), (COL, 0))],
                                          [(TEMP, 0)], 1),
    "no_constraints": encode_program(3, 0, [], 0, [], [], 1),
    "width_zero": encode_program(0, 0, [], 0, [], [(CONST, 0)], 1),
    "width_above_limit": encode_program(33, 0, [], 0, [], [(COL, 0)], 1),
    "temps_above_limit": _hdr(encode_program(3, 0, [], 1, [], [(COL, 0)], 1), n_temps=33),
    "consts_above_limit": encode_program(3, 0, [1] * 65, 0, [], [(COL, 0)], 1),
    "randoms_above_limit": encode_program(3, 65, [], 0, [], [(COL, 0)], 1),
    "constraints_above_limit": encode_program(3, 0, [], 0, [], [(COL, 0)] * 257, 1),
    "instructions_above_limit": encode_program(3, 0, [], 1, [(OP_ADD, 0, (COL, 0), (COL, 0))] * 4097,
                                               [(TEMP, 0)], 1),
    "degree_zero": encode_program(3, 0, [], 0, [], [(COL, 0)], 0),
    "degree_above_limit": encode_program(3, 0, [], 0, [], [(COL, 0)], 8),
    "formal_degree_above_declared": encode_program(3, 0, [], 1, [(OP_MUL, 0, (COL, 0), (COL, 1))],
                                                   [(TEMP, 0)], 1),
    "formal_degree_through_reuse": encode_program(
        3, 0, [], 1, [(OP_MUL, 0, (COL, 0), (COL, 1)), (OP_MUL, 0, (TEMP, 0), (TEMP, 0))], [(TEMP, 0)], 3),
}


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_invalid_program_is_rejected(name):
    assert _create(REJECTED[name]) == INVALID


def test_limits_and_declared_degree_above_formal_are_accepted():
    assert _create(_valid_wire()) == 0
    # every limit at its maximum
    ins = [(OP_ADD, i % 32, (COL, i % 32), (CONST, i % 64)) for i in range(4096)]
    big = encode_program(32, 64, list(range(64)), 32, ins, [(TEMP, i % 32) for i in range(256)], 7)
    assert _create(big) == 0
    # formal degree 1 declared as 3
    assert _create(encode_program(2, 0, [], 1, [(OP_ADD, 0, (COL, 0), (COL, 1))], [(TEMP, 0)], 3)) == 0


@pytest.mark.parametrize("log_rows,randoms,constraints", [(4, 0, 2), (1, 3, 1), (5, 2, 3), (3, 0, 5)])
def test_system_challenges_match_model(log_rows, randoms, constraints):
    seed = b"challenge-set %d %d %d" % (log_rows, randoms, constraints)
    ot, tr = OT.Transcript(), Transcript()
    ot.absorb(seed)
    tr.absorb(seed)
    before = tr.random()
    got = CS.ChallengeSet(tr, randoms, constraints, log_rows)
    assert tr.random() == before == ot.random()  # next_challenge() absorbs nothing
    want = R.System(ot, [None] * constraints, 1, 1, randoms, log_rows)
    assert got.row() == want.challenges.row and len(got.row()) == log_rows
    assert got.trace() == want.challenges.trace
    assert got.constraint() == want.challenges.constraint
    assert got.mask == want.constraint_mask and len(got.mask) == constraints
    if constraints == 1:
        assert got.mask == [1]


@pytest.mark.parametrize("prog", cs_cases.all_programs(), ids=lambda p: p[0])
def test_host_interpreter_matches_callables(prog):
    name, wire, width, randoms, fns = prog
    p = CS.Program(wire)
    assert (p.width, p.n_constraints, p.n_randoms) == (width, len(fns), randoms)
    r = random.Random("interp-" + name)
    rows = [[r.randrange(M) for _ in range(width)] for _ in range(6)]
    rows += [[0] * width, [M - 1] * width]
    for row in rows:
        rnd = [r.randrange(M) for _ in range(randoms)]
        mask = [r.randrange(M) for _ in fns]
        want = sum(mk * f(row, rnd) for mk, f in zip(mask, fns)) % M
        assert p.evaluate(row, rnd, mask) == want


# ---- mlh_cs_sumcheck_verify on proofs made by the model ----------------------

def _model_proof(case):
    """(system, pols, rs, sum, output, transcript at the start, model transcript
    after verification) -- the prover is the plain-Python model."""
    ot = OT.Transcript()
    ot.absorb(case.seed)
    matrix = case.matrix()
    sysm = R.System(ot, case.fns, case.degree, case.width, case.randoms, case.log_height, matrix)
    tables = sysm.build_tables()
    total = sum(d * sysm.evaluate_composition(matrix[i * case.width:(i + 1) * case.width])
                for i, d in enumerate(tables.delta)) % M
    vt = ot.clone()
    pols, rs = sysm.compute_sumcheck_polynomials(ot, tables, total)
    output = R.trace_evaluate(matrix, case.width, rs)
    sysm.verify_with_evaluations(vt, pols, total, output)  # the model accepts its own proof
    assert vt.random() == ot.random()
    return sysm, pols, total, output, vt


VERIFY_CASES = [c for c in cs_cases.cases() if c.log_height <= 5]


@pytest.fixture(scope="module", params=VERIFY_CASES, ids=lambda c: c.name)
def proof(request):
    return (request.param,) + _model_proof(request.param)


def _verify(case, sysm, pols, total, output):
    lib = _lib.load()
    tr = Transcript()
    tr.absorb(case.seed)
    prog = CS.Program(case.wire)
    flat = [c for p in pols for c in p]
    st = lib.mlh_cs_sumcheck_verify(prog.h, len(pols), CS._elems(sysm.challenges.row),
                                    CS._elems(sysm.challenges.trace), CS._elems(sysm.constraint_mask),
                                    CS.fe_bytes(total), CS._elems(flat), CS._elems(output), tr.h)
    return st, tr


def _start_state(case):
    t = OT.Transcript()
    t.absorb(case.seed)
    return t.random()


def test_verify_accepts_model_proof(proof):
    case, sysm, pols, total, output, vt = proof
    st, tr = _verify(case, sysm, pols, total, output)
    assert st == 0
    assert tr.random() == vt.random()  # the model's final transcript state


def test_verify_rejects_flipped_coefficient_byte(proof):
    case, sysm, pols, total, output, _ = proof
    bad = [list(p) for p in pols]
    k = len(bad) // 2
    bad[k][0] ^= 1 << 8  # one bit of byte 1 (the value stays canonical or not: rejected either way)
    st, tr = _verify(case, sysm, bad, total, output)
    assert st == VERIFY
    assert tr.random() == _start_state(case)


def test_verify_rejects_wrong_sum(proof):
    case, sysm, pols, total, output, _ = proof
    st, _ = _verify(case, sysm, pols, (total + 1) % M, output)
    assert st == VERIFY


def test_verify_rejects_wrong_output_element(proof):
    case, sysm, pols, total, output, _ = proof
    bad = list(output)
    bad[-1] = (bad[-1] + 1) % M
    st, _ = _verify(case, sysm, pols, total, bad)
    assert st == VERIFY
