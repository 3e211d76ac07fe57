"""Constraint-system sumcheck on the GPU (cs_sumcheck.hip through the C ABI and
multilinear_amd.constraint_system) against the plain-Python model
tests/cs_reference.py.  Every comparison is bit-exact."""
import ctypes
import functools
import random

import pytest

import cs_cases
import cs_reference as R
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd import polynomials as MP
from multilinear_amd.transcript import Transcript
from oracle import field as F
from oracle import polynomials as OPL
from oracle import transcript as OT

pytestmark = pytest.mark.gpu

M = F.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]
CASES = {c.name: c for c in cs_cases.cases()}


def _true_sum(sysm, matrix, width, delta):
    return sum(d * sysm.evaluate_composition(matrix[i * width:(i + 1) * width])
               for i, d in enumerate(delta)) % M


@functools.lru_cache(maxsize=None)
def model(name):
    """The model's run of a case, computed once: system, matrix, first-round
    tables, sum, proof, final tables and transcript digest."""
    case = CASES[name]
    ot = OT.Transcript()
    ot.absorb(case.seed)
    matrix = case.matrix()
    sysm = R.System(ot, case.fns, case.degree, case.width, case.randoms, case.log_height, matrix)
    tables = sysm.build_tables()
    delta0 = list(tables.delta)
    total = _true_sum(sysm, matrix, case.width, delta0)
    pols, rs = sysm.compute_sumcheck_polynomials(ot, tables, total)
    return dict(sysm=sysm, matrix=matrix, delta0=delta0, total=total, pols=pols, rs=rs,
                final_row=tables.matrix[:case.width], final_delta=tables.delta[0],
                digest=ot.random())


def _dev(values):
    return D.to_device(D.ints_to_limbs(values))


def _host(t):
    return D.limbs_to_ints(D.from_device(t))


def _prove(case, sysm, m, delta, total, tr, width=None, log_height=None, m_null=False):
    lib, ctx = D.lib(), D.context()
    prog = CS.Program(case.wire)
    n = case.log_height if log_height is None else log_height
    Dn = case.degree + 1
    polys = (ctypes.c_uint8 * (16 * Dn * max(n, 1)))()
    rs = (ctypes.c_uint8 * (16 * max(n, 1)))()
    st = lib.mlh_cs_sumcheck_prove(ctx, prog.h, case.width if width is None else width,
                                   None if m_null else D.ptr(m), D.ptr(delta), n,
                                   CS._elems(sysm.challenges.trace), CS._elems(sysm.constraint_mask),
                                   D.fe_bytes(total), tr.h, polys, rs)
    flat = CS._split(polys, Dn * case.log_height)
    return st, [flat[Dn * k:Dn * k + Dn] for k in range(case.log_height)], CS._split(rs, case.log_height)


def _start(case):
    tr = Transcript()
    tr.absorb(case.seed)
    return tr


# ---- the reference's own test system (sumcheck.rs:305-365) --------------------

def test_pythagorean_system():
    matrix = cs_cases.pythagorean_matrix()
    assert len(matrix) == 64
    for i in range(16):
        a, b, c, s = matrix[4 * i:4 * i + 4]
        assert a * a + b * b == c * c and a + b == s
    ot = OT.Transcript()
    sysm = R.System(ot, cs_cases.PYTHAGOREAN_FNS, 2, 4, 0, 4, matrix)
    wt = ot.clone()
    mt = sysm.build_tables()
    want_pols, want_rs = sysm.compute_sumcheck_polynomials(ot, mt, 0)
    sysm.verify_sumcheck_debug(wt, want_pols, 0)

    tr = Transcript()
    cset = CS.ConstraintSet(cs_cases.pythagorean_exprs(), 2)
    layout = CS.WitnessLayout(columns=4, randoms=0)
    trace = CS.Trace(_dev(matrix), 4)
    prover = CS.System.prover(tr, cset, layout, trace)
    vt1, vt2 = tr.clone(), tr.clone()
    tables = prover.build_tables()
    pols, rs = prover.compute_sumcheck_polynomials(tr, tables, 0)
    assert pols == want_pols and rs == want_rs
    assert tr.random() == ot.random()
    prover.verify_sumcheck_debug(vt1, pols, 0)
    assert vt1.random() == tr.random()
    output = MP.trace_evaluate(trace.matrix(), 4, rs)  # the untouched trace at rs
    assert output == R.trace_evaluate(matrix, 4, rs)
    verifier = CS.System.verifier(vt2.clone(), cset, layout, 4)
    verifier.verify_with_evaluations(vt2, pols, 0, output)
    assert vt2.random() == tr.random()
    assert _host(tables.matrix)[:4] == output  # row 0 of the folded matrix
    assert _host(tables.delta)[0] == sysm.evaluate_delta(rs)
    assert _host(trace.matrix()) == matrix  # build_tables cloned it


# ---- random, unsatisfied traces ------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES, key=lambda n: CASES[n].log_height))
def test_prove_matches_model(name):
    case, mo = CASES[name], model(name)
    sysm = mo["sysm"]
    prog = CS.Program(case.wire)
    if case.log_height == 13:
        # more than one block, and a thread visits more than one row pair
        threads, blocks = prog.launch_info(case.log_height)
        print("launch: %d threads x %d blocks for %d row pairs" % (threads, blocks, 1 << 12))
        assert blocks > 1 and (1 << (case.log_height - 1)) > threads * blocks
    if name == "wide32":
        assert max(i[1] for i in _instrs(case.wire)) == 31  # holds all 32 temps
    m = _dev(mo["matrix"])
    delta = MP.eq_table(sysm.challenges.row)
    assert _host(delta) == mo["delta0"]
    tr = _start(case)
    st, pols, rs = _prove(case, sysm, m, delta, mo["total"], tr)
    assert st == 0, D.lib().mlh_last_error(D.context())
    assert rs == mo["rs"]
    assert pols == mo["pols"]
    assert tr.random() == mo["digest"]
    assert _host(m)[:case.width] == mo["final_row"]
    assert _host(delta)[0] == mo["final_delta"]
    # the verifier accepts it with the output from the untouched trace
    output = MP.trace_evaluate(_dev(mo["matrix"]), case.width, rs)
    assert output == mo["final_row"]
    vt = _start(case)
    flat = [c for p in pols for c in p]
    assert D.lib().mlh_cs_sumcheck_verify(prog.h, case.log_height, CS._elems(sysm.challenges.row),
                                          CS._elems(sysm.challenges.trace),
                                          CS._elems(sysm.constraint_mask), D.fe_bytes(mo["total"]),
                                          CS._elems(flat), CS._elems(output), vt.h) == 0
    assert vt.random() == mo["digest"]


def _instrs(wire):
    import struct

    f = struct.unpack("<7I", wire[:28])
    off = 28 + 16 * f[2]
    return [tuple(wire[off + 8 * i:off + 8 * i + 8]) for i in range(f[4])]


# ---- step API ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lin1", "quad3", "deg5_w7", "wide32"])
def test_step_api_matches_model(name):
    case, mo = CASES[name], model(name)
    sysm, W, L, Dn = mo["sysm"], case.width, case.log_height, case.degree + 1
    lib, ctx = D.lib(), D.context()
    prog = CS.Program(case.wire)
    rnd, mask = CS._elems(sysm.challenges.trace), CS._elems(sysm.constraint_mask)
    tab = R.SumcheckTables(list(mo["matrix"]), W, 1 << L, list(mo["delta0"]))
    comp = sysm.evaluate_composition
    m, d = _dev(mo["matrix"]), _dev(mo["delta0"])
    out = (ctypes.c_uint8 * (16 * Dn))()
    D.check(lib.mlh_cs_partial_sums(ctx, prog.h, W, D.ptr(m), D.ptr(d), L, rnd, mask, out), ctx)
    assert CS._split(out, Dn) == [tab.partial_sum(comp, F.from_i64(x)) for x in range(1, Dn + 1)]
    assert _host(m) == mo["matrix"] and _host(d) == mo["delta0"]  # read only
    r = random.Random("step-" + name).randrange(M)
    if L >= 2:  # fold + the folded tables' sums, one pass
        m2, d2 = _dev(mo["matrix"]), _dev(mo["delta0"])
        D.check(lib.mlh_cs_fold_and_sums(ctx, prog.h, W, D.ptr(m2), D.ptr(d2), L, rnd, mask,
                                         D.fe_bytes(r), out), ctx)
    D.check(lib.mlh_cs_fold(ctx, W, D.ptr(m), D.ptr(d), L, D.fe_bytes(r)), ctx)
    tab.fold(r)
    half = 1 << (L - 1)
    assert _host(m)[:half * W] == tab.matrix and _host(d)[:half] == tab.delta
    if L >= 2:
        assert _host(m2)[:half * W] == tab.matrix and _host(d2)[:half] == tab.delta
        assert CS._split(out, Dn) == [tab.partial_sum(comp, F.from_i64(x)) for x in range(1, Dn + 1)]


# ---- agreement with the width-1 path ---------------------------------------------

def test_width1_x0_program_equals_pcs_sumcheck():
    L = 10
    r = random.Random("cs-x0")
    ev = [r.randrange(M) for _ in range(1 << L)]
    pts = [r.randrange(M) for _ in range(L)]
    total = OPL.mle_evaluate(ev, pts)
    lib, ctx = D.lib(), D.context()

    m1, d1, t1 = _dev(ev), MP.eq_table(pts), Transcript()
    p1 = (ctypes.c_uint8 * (32 * L))()
    r1 = (ctypes.c_uint8 * (16 * L))()
    D.check(lib.mlh_sumcheck_prove(ctx, D.ptr(m1), D.ptr(d1), L, D.fe_bytes(total), t1.h, p1, r1), ctx)

    prog = CS.Program(CS.compile_program([CS.var(0)], 1, 0, 1))
    m2, d2, t2 = _dev(ev), MP.eq_table(pts), Transcript()
    p2 = (ctypes.c_uint8 * (32 * L))()
    r2 = (ctypes.c_uint8 * (16 * L))()
    D.check(lib.mlh_cs_sumcheck_prove(ctx, prog.h, 1, D.ptr(m2), D.ptr(d2), L, None, CS._elems([1]),
                                      D.fe_bytes(total), t2.h, p2, r2), ctx)
    assert bytes(p2) == bytes(p1)
    assert bytes(r2) == bytes(r1)
    assert t2.random() == t1.random()
    assert _host(m2)[0] == _host(m1)[0] and _host(d2)[0] == _host(d1)[0]


# ---- argument errors -------------------------------------------------------------

@pytest.mark.parametrize("what", ["width_mismatch", "null_matrix", "log_height_above_max"])
def test_argument_errors_leave_transcript_unchanged(what):
    case, mo = CASES["quad3"], model("quad3")
    m, delta = _dev(mo["matrix"]), _dev(mo["delta0"])
    tr = _start(case)
    before = tr.random()
    kw = {"width_mismatch": dict(width=case.width + 1), "null_matrix": dict(m_null=True),
          "log_height_above_max": dict(log_height=33)}[what]
    st, _, _ = _prove(case, mo["sysm"], m, delta, mo["total"], tr, **kw)
    assert st == INVALID
    assert tr.random() == before
    assert _host(m) == mo["matrix"] and _host(delta) == mo["delta0"]


def test_zero_rounds():
    case, mo = CASES["lin1"], model("lin1")
    m, delta = _dev(mo["matrix"][:1]), _dev([1])
    tr = _start(case)
    before = tr.random()
    st, _, _ = _prove(case, mo["sysm"], m, delta, mo["total"], tr, log_height=0)
    assert st == 0 and tr.random() == before
    assert _host(m) == mo["matrix"][:1] and _host(delta) == [1]
