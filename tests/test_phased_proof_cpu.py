"""The host side of the two-phase system proof on the proofs of the
plain-Python model tests/phased_reference.py: mlh_system_trace_randoms,
mlh_cs_sumcheck_verify_sums and mlh_system_verify_phased.  Accepted with the
model's transcript digest; rejected with MLH_ERR_VERIFY and an untouched
transcript for every altered field.  Runs without a GPU."""
import ctypes

import pytest

import phased_reference as PR
import system_reference as S
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.transcript import Transcript
from oracle import field as F

M = F.M
VERIFY = _lib.STATUS_CODES["MLH_ERR_VERIFY"]
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]
CPU_NAMES = ["lin1", "quad3", "pythagorean", "deg5_w7", "wide32"]  # up to 2^9 rows


def _start(mo):
    tr = Transcript()
    tr.absorb(mo["seed"])
    return tr


def _elems(vals):
    return CS._elems(vals)


# ---- mlh_system_trace_randoms ---------------------------------------------------

@pytest.mark.parametrize("name", ["quad3", "deg5_w7", "pythagorean"])
def test_trace_randoms_match_model_and_leave_transcript(name):
    mo = PR.model(name)
    tr = _start(mo)
    n = mo["randoms"]
    out = (ctypes.c_uint8 * (16 * max(n, 1)))()
    root = (ctypes.c_uint8 * 32).from_buffer_copy(mo["root1"])
    assert D.lib().mlh_system_trace_randoms(tr.h, root, n, out) == 0
    assert CS._split(out, n) == mo["trace_randoms"]
    assert tr.random() == mo["entry"]
    if n:
        assert D.lib().mlh_system_trace_randoms(tr.h, root, n, None) == INVALID
    assert D.lib().mlh_system_trace_randoms(tr.h, None, n, out) == INVALID
    assert D.lib().mlh_system_trace_randoms(None, root, n, out) == INVALID


# ---- mlh_cs_sumcheck_verify_sums ------------------------------------------------

def _verify_sums(name, mo, mask=None, beta=None, claim=None):
    prog = CS.Program(S.program_wire(name))
    # the transcript as the rounds found it: the model's state before the sumcheck
    tr = _replay_to_sumcheck(mo)
    before = tr.random()
    assert before == mo["before_sumcheck"].random()
    ch = mo["sysm"].challenges
    mask = mo["mask"] if mask is None else mask
    beta = mo["beta"] if beta is None else beta
    claim = mo["claim"] if claim is None else claim
    flat = [c for p in mo["pols"] for c in p]
    st = D.lib().mlh_cs_sumcheck_verify_sums(prog.h, mo["log_height"], _elems(ch.row),
                                             _elems(ch.trace), _elems(mo["sysm"].constraint_mask),
                                             mask, D.fe_bytes(beta), D.fe_bytes(claim), _elems(flat),
                                             _elems(mo["output"]), tr.h)
    return st, tr.random(), before


def _replay_to_sumcheck(mo):
    tr = _start(mo)
    tr.absorb(mo["root1"])
    if mo["root2"] is not None:
        tr.absorb(mo["root2"])
    if mo["sum_columns"]:
        tr.absorb(F.to_bytes(mo["column_sum"]))
    return tr


@pytest.mark.parametrize("name", CPU_NAMES)
def test_verify_sums_accepts_model_rounds(name):
    mo = PR.model(name)
    st, digest, _ = _verify_sums(name, mo)
    assert st == 0
    assert digest == mo["after_sumcheck"]


@pytest.mark.parametrize("name", ["lin1", "quad3", "deg5_w7", "wide32"])
def test_verify_sums_rejects_wrong_beta_mask_claim(name):
    mo = PR.model(name)
    assert mo["mask"] and mo["beta"]
    st, digest, before = _verify_sums(name, mo, beta=(mo["beta"] + 1) % M)
    assert st == VERIFY and digest == before
    other = mo["mask"] ^ 1  # column 0 in or out of the sum
    if other:
        st, digest, before = _verify_sums(name, mo, mask=other)
        assert st == VERIFY and digest == before
    st, digest, before = _verify_sums(name, mo, mask=0)  # no sum term at all
    assert st == VERIFY and digest == before
    st, digest, before = _verify_sums(name, mo, claim=(mo["claim"] + 1) % M)
    assert st == VERIFY and digest == before
    if mo["width"] < 32:  # a bit at or above the width is an argument error
        st, digest, before = _verify_sums(name, mo, mask=mo["mask"] | (1 << mo["width"]))
        assert st == INVALID and digest == before


def test_verify_sums_mask_zero_is_the_plain_verifier():
    name = "pythagorean"
    mo = PR.model(name)
    assert mo["mask"] == 0 and mo["claim"] == mo["total"]
    st, digest, _ = _verify_sums(name, mo)
    assert st == 0
    prog = CS.Program(S.program_wire(name))
    tr = _replay_to_sumcheck(mo)
    ch = mo["sysm"].challenges
    flat = [c for p in mo["pols"] for c in p]
    assert D.lib().mlh_cs_sumcheck_verify(prog.h, mo["log_height"], _elems(ch.row), _elems(ch.trace),
                                          _elems(mo["sysm"].constraint_mask),
                                          D.fe_bytes(mo["total"]), _elems(flat),
                                          _elems(mo["output"]), tr.h) == 0
    assert tr.random() == digest


# ---- mlh_system_verify_phased ---------------------------------------------------

def _verify(name, mo, p, pre=None, mask=None, total=None, column_sum=None, log_height=None):
    prog = CS.Program(S.program_wire(name))
    tr = _start(mo)
    assert tr.random() == mo["entry"]
    st = D.lib().mlh_system_verify_phased(
        prog.h, mo["log_height"] if log_height is None else log_height,
        mo["pre"] if pre is None else pre, mo["mask"] if mask is None else mask,
        D.fe_bytes(mo["total"] if total is None else total),
        D.fe_bytes(mo["column_sum"] if column_sum is None else column_sum), ctypes.byref(p.c), tr.h)
    return st, tr.random()


@pytest.mark.parametrize("name", CPU_NAMES)
def test_verifier_accepts_model_proof(name):
    mo = PR.model(name)
    st, digest = _verify(name, mo, PR.pack(mo))
    assert st == 0
    assert digest == mo["digest"]


def test_one_phase_no_sums_is_the_system_proof():
    """P = W, S empty: the model's phased proof is the model's system proof."""
    mo, so = PR.model("pythagorean"), S.model("pythagorean")
    assert mo["root1"] == so["root"] and mo["pols"] == so["pols"] and mo["output"] == so["output"]
    assert mo["pcs"][0] == so["pcs"] and mo["digest"] == so["digest"]


def _flip(buf, i):
    buf[i] ^= 1


def _swap_pcs(p):
    a = _lib.BatchedPcsProofC.from_buffer_copy(p.c.pcs[0])
    p.c.pcs[0] = p.c.pcs[1]
    p.c.pcs[1] = a


MUTATIONS = {
    "root1_byte": lambda p, mo: _flip(p.c.pcs[0].fri.batch_commitment, 7),
    "root2_byte": lambda p, mo: _flip(p.c.pcs[1].fri.batch_commitment, 9),
    "sumcheck_coefficient_byte": lambda p, mo: _flip(p._polys, len(p._polys) - 9),
    "output_byte_below_P": lambda p, mo: _flip(p._output, 3),
    "output_byte_at_P": lambda p, mo: _flip(p._output, 16 * mo["pre"] + 3),
    "opening1_coefficient_byte": lambda p, mo: _flip(p.pcs[0]._polys, 17 % len(p.pcs[0]._polys)),
    "opening2_coefficient_byte": lambda p, mo: _flip(p.pcs[1]._polys, 17 % len(p.pcs[1]._polys)),
    "opening1_query_byte": lambda p, mo: _flip(p.pcs[0].fri_proof._q,
                                               5 * p.pcs[0].fri_proof.qbytes + 40),
    "opening2_query_byte": lambda p, mo: _flip(p.pcs[1].fri_proof._q,
                                               5 * p.pcs[1].fri_proof.qbytes + 40),
    "swapped_openings": lambda p, mo: _swap_pcs(p),
    "pre_random_header": lambda p, mo: setattr(p.c, "pre_random_columns", p.c.pre_random_columns + 1),
    "mask_header": lambda p, mo: setattr(p.c, "sum_column_mask", p.c.sum_column_mask ^ 2),
    "width_header": lambda p, mo: setattr(p.c, "width", p.c.width + 1),
    "non_canonical_output": lambda p, mo: ctypes.memmove(p._output, b"\xff" * 16, 16),
    "non_canonical_coefficient": lambda p, mo: ctypes.memmove(p._polys, M.to_bytes(16, "little"), 16),
}


@pytest.mark.parametrize("what", sorted(MUTATIONS))
@pytest.mark.parametrize("name", ["quad3", "deg5_w7"])  # two commitments each
def test_verifier_rejects_altered_proof(name, what):
    mo = PR.model(name)
    p = PR.pack(mo)
    MUTATIONS[what](p, mo)
    st, digest = _verify(name, mo, p)
    assert st == VERIFY
    assert digest == mo["entry"]  # the transcript is as it was, the roots included


@pytest.mark.parametrize("name", ["quad3", "deg5_w7", "wide32"])
def test_verifier_rejects_wrong_public_inputs(name):
    mo = PR.model(name)
    p = PR.pack(mo)
    W = mo["width"]
    for pre in {mo["pre"] - 1, mo["pre"] + 1, 0, W, W + 1} - {mo["pre"]}:
        st, digest = _verify(name, mo, p, pre=pre)
        assert st == VERIFY and digest == mo["entry"], pre
    for mask in (0, mo["mask"] ^ 1, mo["mask"] ^ (1 << (W - 1))):
        if mask != mo["mask"]:
            st, digest = _verify(name, mo, p, mask=mask)
            assert st == VERIFY and digest == mo["entry"], mask
    st, digest = _verify(name, mo, p, column_sum=(mo["column_sum"] + 1) % M)
    assert st == VERIFY and digest == mo["entry"]
    st, digest = _verify(name, mo, p, total=(mo["total"] + 1) % M)
    assert st == VERIFY and digest == mo["entry"]
    # sum and column_sum traded so that sum + beta * column_sum is NOT preserved
    # (beta is drawn after column_sum is absorbed)
    st, digest = _verify(name, mo, p, total=(mo["total"] + mo["beta"]) % M,
                         column_sum=(mo["column_sum"] - 1) % M)
    assert st == VERIFY and digest == mo["entry"]
    for lh in (mo["log_height"] + 1, mo["log_height"] - 1):
        st, digest = _verify(name, mo, p, log_height=lh)
        assert st == VERIFY and digest == mo["entry"]
    st, digest = _verify(name, mo, p)  # the untouched proof still verifies
    assert st == 0 and digest == mo["digest"]
