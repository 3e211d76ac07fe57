"""The committed random programs of tests/program_fuzz.py on the GPU: the
constraint interpreter of csrc/cs_sumcheck.hip (partial sums, fold and sums,
the whole prover, with and without sum columns) against tests/cs_reference.py
and tests/phased_reference.py run on the generators' closures, and the fill
interpreter of csrc/trace_fill.hip against the generators' own row functions
and the host interpreter.  Every comparison is bit-exact."""
import ctypes
import random

import pytest

import cs_reference as R
import phased_reference as PR
import program_fuzz as PF
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd import polynomials as MP
from multilinear_amd.transcript import Transcript
from oracle import field as F
from oracle import transcript as OT

pytestmark = pytest.mark.gpu

M = F.M


def _ids(table):
    return ["%s%d" % (e["kind"], e["seed"]) for e in table]


def _dev(values):
    return D.to_device(D.ints_to_limbs(values))


def _host(t):
    return D.limbs_to_ints(D.from_device(t))


# ---- constraint programs ------------------------------------------------------------

def cs_model(entry):
    """The case, its system with distinct random challenges and mask (the
    reference draws one challenge for all of them, which would hide a wrong
    random or mask index), the matrix and the true sum."""
    case = PF.cs_case(entry)
    W, L = case.width, entry["log_height"]
    r = random.Random("gpu %s" % case.name)
    seed = bytes(r.randrange(256) for _ in range(r.randrange(0, 40)))
    matrix = PF.matrix(case.name, 1 << L, W)
    ot = OT.Transcript()
    ot.absorb(seed)
    sysm = R.System(ot, case.fns, case.degree, W, case.n_randoms, L, matrix)
    sysm.challenges.row = [r.randrange(M) for _ in range(L)]
    sysm.challenges.trace = [r.randrange(M) for _ in range(case.n_randoms)]
    sysm.constraint_mask = [r.randrange(M) for _ in range(case.n_constraints)]
    delta = sysm.build_tables().delta
    total = sum(d * sysm.evaluate_composition(matrix[i * W:(i + 1) * W])
                for i, d in enumerate(delta)) % M
    return dict(case=case, seed=seed, ot=ot, sysm=sysm, matrix=matrix, delta=delta, total=total,
                rng=r)


def _sums(tab, comp, Dn):
    return [tab.partial_sum(comp, F.from_i64(x)) for x in range(1, Dn + 1)]


def _check_steps(mo, prog, L, fold):
    """mlh_cs_partial_sums on the first 2^L rows of the matrix and of delta (any
    table will do for delta), and mlh_cs_fold_and_sums when asked."""
    case, sysm = mo["case"], mo["sysm"]
    W, Dn = case.width, case.degree + 1
    lib, ctx = D.lib(), D.context()
    rnd, mask = CS._elems(sysm.challenges.trace), CS._elems(sysm.constraint_mask)
    comp = sysm.evaluate_composition
    matrix, delta = mo["matrix"][:W << L], mo["delta"][:1 << L]
    tab = R.SumcheckTables(list(matrix), W, 1 << L, list(delta))
    m, d = _dev(matrix), _dev(delta)
    out = (ctypes.c_uint8 * (16 * Dn))()
    D.check(lib.mlh_cs_partial_sums(ctx, prog.h, W, D.ptr(m), D.ptr(d), L, rnd, mask, out), ctx)
    assert CS._split(out, Dn) == _sums(tab, comp, Dn), (case.name, L)
    assert _host(m) == matrix and _host(d) == delta  # read only
    if fold:
        rng = mo["rng"]
        r = rng.randrange(M) if rng.random() < 0.7 else rng.choice([0, 1, M - 1])
        D.check(lib.mlh_cs_fold_and_sums(ctx, prog.h, W, D.ptr(m), D.ptr(d), L, rnd, mask,
                                         D.fe_bytes(r), out), ctx)
        tab.fold(r)
        half = 1 << (L - 1)
        assert _host(m)[:half * W] == tab.matrix and _host(d)[:half] == tab.delta
        assert CS._split(out, Dn) == _sums(tab, comp, Dn), (case.name, L, "fold")


@pytest.mark.parametrize("entry", PF.CS_TABLE, ids=_ids(PF.CS_TABLE))
def test_constraint_program_matches_model(entry):
    mo = cs_model(entry)
    case, sysm, ot = mo["case"], mo["sysm"], mo["ot"]
    W, L, Dn = case.width, entry["log_height"], case.degree + 1
    lib, ctx = D.lib(), D.context()
    prog = CS.Program(case.wire)
    assert prog.launch_info(L)[0] == entry["threads"]
    for l in sorted({1, 2, 5} | ({L} if not entry["small"] else set())):
        _check_steps(mo, prog, l, fold=(l == L and not entry["small"]))
    # the whole prover on the model's transcript
    smask = PF.sum_mask(entry, W)
    cols = [j for j in range(W) if (smask >> j) & 1]
    beta = mo["rng"].randrange(M) if smask else 0
    column_sum = sum(mo["matrix"][i * W + j] for i in range(1 << L) for j in cols) % M
    claim = (mo["total"] + beta * column_sum) % M
    if smask:
        pols, rs, final_row = PR.sumcheck(sysm, ot, cols, beta, claim)
    else:
        tables = sysm.build_tables()
        pols, rs = sysm.compute_sumcheck_polynomials(ot, tables, claim)
        final_row = tables.matrix[:W]
    m, delta = _dev(mo["matrix"]), MP.eq_table(sysm.challenges.row)
    assert _host(delta) == mo["delta"]
    tr = Transcript()
    tr.absorb(mo["seed"])
    vt = tr.clone()
    polys = (ctypes.c_uint8 * (16 * Dn * L))()
    rs_out = (ctypes.c_uint8 * (16 * L))()
    rnd, mask = CS._elems(sysm.challenges.trace), CS._elems(sysm.constraint_mask)
    if smask:
        st = lib.mlh_cs_sumcheck_prove_sums(ctx, prog.h, W, D.ptr(m), D.ptr(delta), L, rnd, mask,
                                            smask, D.fe_bytes(beta), D.fe_bytes(claim), tr.h, polys,
                                            rs_out)
    else:
        st = lib.mlh_cs_sumcheck_prove(ctx, prog.h, W, D.ptr(m), D.ptr(delta), L, rnd, mask,
                                       D.fe_bytes(claim), tr.h, polys, rs_out)
    assert st == 0, lib.mlh_last_error(ctx)
    flat = CS._split(polys, Dn * L)
    assert [flat[Dn * k:Dn * k + Dn] for k in range(L)] == pols
    assert CS._split(rs_out, L) == rs
    assert tr.random() == ot.random()
    assert _host(m)[:W] == final_row
    assert _host(delta)[0] == sysm.evaluate_delta(rs)
    # the verifier accepts it with the output from the untouched trace
    output = MP.trace_evaluate(_dev(mo["matrix"]), W, rs)
    assert output == final_row
    row = CS._elems(sysm.challenges.row)
    if smask:
        st = lib.mlh_cs_sumcheck_verify_sums(prog.h, L, row, rnd, mask, smask, D.fe_bytes(beta),
                                             D.fe_bytes(claim), CS._elems(flat), CS._elems(output),
                                             vt.h)
    else:
        st = lib.mlh_cs_sumcheck_verify(prog.h, L, row, rnd, mask, D.fe_bytes(claim),
                                        CS._elems(flat), CS._elems(output), vt.h)
    assert st == 0
    assert vt.random() == ot.random()


# ---- fill programs -------------------------------------------------------------------

def _run_fill(case, prog, log_height, shape):
    W, h = case.width, 1 << log_height
    rnd = case.randoms()
    B, K = shape if shape else prog.launch_info(log_height)[:2]
    matrix = case.matrix(log_height, B, K)
    m = _dev(matrix)
    ctx = D.context()
    if shape is None:
        assert CS.Trace(m, W).fill(prog, rnd) is prog
    else:
        st = D.lib().mlh_trace_fill_shaped(ctx, prog.h, D.ptr(m), log_height, W, CS._elems(rnd), B, K)
        assert st == 0, D.lib().mlh_last_error(ctx)
    got = _host(m)
    tag = (case.name, log_height, shape)
    assert got == case.fill_matrix(matrix, rnd), tag
    for j in range(W):  # a column that is no output is untouched
        if not (prog.output_mask >> j) & 1:
            assert got[j::W] == matrix[j::W], tag
    for i in range(h):
        assert got[i * W:(i + 1) * W] == prog.evaluate(matrix[i * W:(i + 1) * W], rnd), (tag, i)


@pytest.mark.parametrize("entry", PF.FILL_TABLE, ids=_ids(PF.FILL_TABLE))
def test_fill_program_matches_model(entry):
    case = PF.fill_table_case(entry)
    prog = CS.FillProgram(case.wire)
    assert prog.n_inverses == entry["n_inv"]
    assert prog.launch_info(entry["log_height"]) == (entry["threads"], 1, 1)
    _run_fill(case, prog, 0, None)
    _run_fill(case, prog, entry["log_height"], None)
    for B, K, L in entry["shapes"]:
        _run_fill(case, prog, L, (B, K))
