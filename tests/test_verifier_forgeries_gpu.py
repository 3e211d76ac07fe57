"""The device provers made to cheat.  They take their challenges and claims
from the caller, so the lies of tests/forge_reference.py that a caller can
tell can be told on the GPU: a fold with a challenge the transcript did not
draw (the step API), and a false claim through the full provers (PCS, batched
PCS, the system proof, the phased proof; the PCS also with the fused rounds
switched off).  Every device proof is byte for byte the CPU forger's (or the
model's / the C oracle's) proof of the same lie, and the host verifier
rejects it at the one check explain() names."""
import ctypes
import functools

import pytest

import forge_reference as FR
import phased_reference as PR
import system_reference as S
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd import fri as MF
from multilinear_amd import multilinear_pcs as MP
from multilinear_amd.batched import BatchedFriProverData, BatchedPCSProof
from multilinear_amd.transcript import Transcript
from oracle import batched as OB
from oracle import coracle as OC
from oracle import field as F
from oracle import fri as OF
from oracle import pcs as OP
from oracle import transcript as OT
from test_gpu_pcs_fused import fused_max
from test_phased_proof_gpu import _prove as phased_prove
from test_system_proof_gpu import _assert_pcs_equals_model
from test_system_proof_gpu import _prove as system_prove
from test_verifier_forgeries_cpu import VERIFY, c_verdict

pytestmark = pytest.mark.gpu

M = F.M


def dev(values):
    return D.to_device(D.ints_to_limbs(values))


def _draw(tr, domain):
    """The query indices of every prove() (fri/mod.rs:268-277) on a host transcript."""
    out = []
    for _ in range(_lib.NUM_QUERIES):
        idx = int.from_bytes(tr.random()[:8], "little") % (domain // 2)
        out.append(idx)
        tr.absorb(idx.to_bytes(8, "little"))
    return out


def _rejected_at(kind, shape, lie, proof, expect, start=None):
    """The assembled proof is the C verifier's MLH_ERR_VERIFY, with and
    without query_indices, and explain() names exactly `expect`."""
    member = FR.Member(kind, shape, lie, proof, expect, start)
    assert member.explain() == expect
    assert c_verdict(D.lib(), member, indices=True) == VERIFY
    assert c_verdict(D.lib(), member) == VERIFY


# ---- wrong_challenge through the step API ---------------------------------------------

@pytest.mark.parametrize("log_n,k", [(ln, k) for ln in (1, 2, 3, 7) for k in range(ln)])
def test_fri_fold_step_with_a_challenge_not_drawn(log_n, k):
    L, lie = log_n + 1, ("wrong_challenge", k)
    gp = F.pow_2_generator_powers(L)
    code = OF.reed_solomon(FR.rand_vals(700 + log_n, 1 << log_n), gp[1])
    want = FR.forge_fri(code, gp, OT.Transcript(), lie)
    tr, dcode = Transcript(), dev(code)
    pd = MF.FriProverData.init(dcode, tr)
    for s in range(log_n):
        r = tr.next_challenge()
        pd.fold_step(s, (r + 1) % M if s == k else r, tr)
    indices = _draw(tr, 1 << L)
    raw = b"".join(v + b"".join(sibs) for q in pd.open_queries(indices, L) for v, sibs in q)
    assert pd.fold_roots() == want.commitments
    assert pd.last_element == want.last_elem
    assert tr.random() == want.last_random  # the transcript digest
    assert indices == FR.opened_indices(want)
    got = FR.fri_from_flat(pd.fold_roots(), raw, indices, pd.last_element, tr.random())
    assert FR.proof_bytes(got) == FR.proof_bytes(want)  # every opened record
    _rejected_at("fri", (log_n,), lie, got, {FR.fold_check(k, log_n)})


@pytest.mark.parametrize("m,log_n", [(2, 1), (3, 2), (2, 7)])
def test_batched_fold_step_with_a_challenge_not_drawn(m, log_n):
    L, lie = log_n + 1, ("wrong_challenge", 0)
    gp = F.pow_2_generator_powers(L)
    codes = [OF.reed_solomon(FR.rand_vals(720 + 10 * log_n + j, 1 << log_n), gp[1]) for j in range(m)]
    want = FR.forge_batched_fri(codes, gp, OT.Transcript(), lie)
    tr, dcodes = Transcript(), dev([v for c in codes for v in c])
    bp = BatchedFriProverData.init(dcodes, m, tr)
    r = tr.next_challenge()
    bp.batched_fold_step((gp[1], L), (r + 1) % M, tr)
    fd = bp.fri_data
    for k in range(1, log_n):
        fd.fold_step(k, tr.next_challenge(), tr, gen_pows=(gp[1], L))
    indices = _draw(tr, 1 << L)
    raw = b"".join(bp.open_query_at(i) for i in indices)
    assert bp.batch_root == want.batch_commitment and fd.fold_roots() == want.commitments
    assert fd.last_element == want.last_elem
    assert tr.random() == want.last_random
    got = FR.batched_from_flat(bp.batch_root, fd.fold_roots(), m, raw, indices, fd.last_element,
                               tr.random())
    assert FR.proof_bytes(got) == FR.proof_bytes(want)
    _rejected_at("batched_fri", (m, log_n), lie, got, {FR.fold_check(0, log_n, True)})


# ---- wrong_claim through the full provers ---------------------------------------------

@functools.lru_cache(maxsize=None)
def _pcs_case(n):
    """-> (points, evals, true output, the proof of output + 1): the CPU
    forger's up to 2^9, the C oracle's above (as system_reference._open)."""
    pts, ev = FR.rand_vals(800 + n, n), FR.rand_vals(810 + n, 1 << n)
    if n <= S.PY_MAX_LOG:
        out = FR._mle(ev, pts)
        return pts, ev, out, FR.forge_pcs(pts, out, ev, OT.Transcript(), ("wrong_claim",))
    limbs = S._limbs(ev)
    out = OC.mle_evaluate_par(limbs, n, pts)
    cp = OC.pcs_prove_par(limbs, n, pts, [(out + 1) % M])
    assert cp["rc"] == 0
    fp = FR.fri_from_flat(cp["roots"], cp["queries"], cp["indices"], cp["last_elem"], cp["last_random"])
    return pts, ev, out, OP.PCSProof(fp, [tuple(p) for p in cp["polys"]], list(pts), (out + 1) % M)


def _pcs_wrong_claim(n):
    pts, ev, out, want = _pcs_case(n)
    claim = (out + 1) % M
    p = MP.PCSProof.prove(pts, claim, dev(ev), Transcript())
    fp = p.fri_proof
    got = OP.PCSProof(FR.fri_from_flat(fp.commitments, bytes(fp._q), fp.query_indices, fp.last_elem,
                                       fp.last_random), p.sumcheck_polynomials, list(pts), claim)
    assert FR.proof_bytes(got) == FR.proof_bytes(want)
    assert not p.verify(Transcript())
    _rejected_at("pcs", (n,), ("wrong_claim",), got, {"K6"})


@pytest.mark.parametrize("n", [1, 2, 8, 13])
def test_pcs_prove_of_a_false_claim(n):
    _pcs_wrong_claim(n)


@pytest.mark.parametrize("n", [2, 8])
def test_pcs_prove_of_a_false_claim_cooperative_rounds(n):
    with fused_max(0):
        _pcs_wrong_claim(n)


@pytest.mark.parametrize("m,n,j", [(2, 1, 0), (2, 1, 1), (3, 5, 0), (3, 5, 1), (3, 5, 2)])
def test_batched_pcs_prove_of_a_false_claim(m, n, j):
    lie = ("wrong_claim", j)
    pts = FR.rand_vals(830 + n, n)
    polys = [FR.rand_vals(840 + 10 * n + i, 1 << n) for i in range(m)]
    outs = [FR._mle(p, pts) for p in polys]
    want = FR.forge_batched_pcs(pts, outs, polys, OT.Transcript(), lie)
    claimed = list(want.outputs)
    assert claimed[j] == (outs[j] + 1) % M
    p = BatchedPCSProof.prove(pts, claimed, dev([v for q in polys for v in q]), Transcript())
    fp = p.fri_proof
    got = OB.BatchedPCSProof(
        FR.batched_from_flat(fp.batch_commitment, fp.commitments, m, bytes(fp._q), fp.query_indices,
                             fp.last_elem, fp.last_random),
        p.sumcheck_polynomials, list(pts), claimed)
    assert FR.proof_bytes(got) == FR.proof_bytes(want)
    assert not p.verify(Transcript())
    _rejected_at("batched_pcs", (m, n), lie, got, {"K6"})


@pytest.mark.parametrize("name", FR.SYSTEM_NAMES)
def test_system_prove_of_a_false_total(name):
    mo, total, expect = FR.system_forgery(name, "wrong_total_consistent")
    assert mo["total"] == total == (S.model(name)["total"] + 1) % M and expect == {"K10"}
    tr = Transcript()
    tr.absorb(mo["seed"])
    entry = tr.clone()
    st, p, _ = system_prove(name, mo, tr)  # proves mo["total"]
    assert st == 0, D.lib().mlh_last_error(D.context())
    assert p.sumcheck_polynomials == mo["pols"] and p.output == mo["output"]
    _assert_pcs_equals_model(p.pcs, mo["pcs"])
    assert tr.random() == mo["digest"]
    assert FR.explain_system(mo, total) == expect
    prog = CS.Program(S.program_wire(name))
    assert D.lib().mlh_system_verify(prog.h, mo["log_height"], D.fe_bytes(total), ctypes.byref(p.c),
                                     entry.h) == VERIFY
    assert entry.random() == mo["entry"]


@pytest.mark.parametrize("lie", ["wrong_total_consistent", "wrong_column_sum_consistent"])
@pytest.mark.parametrize("name", ["lin1", "quad3"])  # P = W and P < W
def test_phased_prove_of_a_false_sum(name, lie):
    mo, total, column_sum, expect = FR.phased_forgery(name, lie)
    assert (mo["total"], mo["column_sum"]) == (total, column_sum) and expect == {"K10"}
    honest = PR.model(name)
    assert (total, column_sum) != (honest["total"], honest["column_sum"])
    tr = Transcript()
    tr.absorb(mo["seed"])
    entry = tr.clone()
    st, p, _ = phased_prove(name, mo, tr)  # proves mo["total"], mo["column_sum"]
    assert st == 0, D.lib().mlh_last_error(D.context())
    assert p.sumcheck_polynomials == mo["pols"] and p.output == mo["output"]
    assert len(p.pcs) == len(mo["pcs"])
    for got, want in zip(p.pcs, mo["pcs"]):
        _assert_pcs_equals_model(got, want)
    assert tr.random() == mo["digest"]
    assert FR.explain_system(mo, total, column_sum) == expect
    prog = CS.Program(S.program_wire(name))
    assert D.lib().mlh_system_verify_phased(prog.h, mo["log_height"], mo["pre"], mo["mask"],
                                            D.fe_bytes(total), D.fe_bytes(column_sum),
                                            ctypes.byref(p.c), entry.h) == VERIFY
    assert entry.random() == mo["entry"]
