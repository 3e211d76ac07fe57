"""mlh_system_verify (host only) on the proofs of the plain-Python model
tests/system_reference.py: accepted with the model's transcript digest;
rejected with MLH_ERR_VERIFY and an untouched transcript for every altered
field.  Runs without a GPU."""
import ctypes

import pytest

import system_reference as S
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.transcript import Transcript
from oracle import field as F

VERIFY = _lib.STATUS_CODES["MLH_ERR_VERIFY"]
CPU_NAMES = ["pythagorean", "lin1", "quad3", "deg5_w7"]
NEW_SYMBOLS = ["mlh_trace_columns", "mlh_trace_columns_launch_info", "mlh_trace_commit",
               "mlh_trace_commitment_root", "mlh_trace_commitment_width",
               "mlh_trace_commitment_log_height", "mlh_trace_commitment_destroy",
               "mlh_system_prove", "mlh_system_verify"]


def _start(mo):
    tr = Transcript()
    tr.absorb(mo["seed"])
    return tr


def _verify(name, mo, p, total=None, log_height=None):
    prog = CS.Program(S.program_wire(name))
    tr = _start(mo)
    assert tr.random() == mo["entry"]
    st = D.lib().mlh_system_verify(prog.h, mo["log_height"] if log_height is None else log_height,
                                   D.fe_bytes(mo["total"] if total is None else total),
                                   ctypes.byref(p.c), tr.h)
    return st, tr.random()


def test_new_symbols_are_exported():
    lib = D.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES


@pytest.mark.parametrize("name", CPU_NAMES)
def test_verifier_accepts_model_proof(name):
    mo = S.model(name)
    if name == "pythagorean":
        assert (mo["log_height"], mo["width"], mo["total"], mo["seed"]) == (4, 4, 0, b"")
    st, digest = _verify(name, mo, S.pack(mo))
    assert st == 0
    assert digest == mo["digest"]


def _flip(buf, i):
    buf[i] ^= 1


MUTATIONS = {
    "output_byte": lambda p: _flip(p._output, 3),
    "sumcheck_coefficient_byte": lambda p: _flip(p._polys, len(p._polys) - 9),
    "batch_commitment_byte": lambda p: _flip(p.c.pcs.fri.batch_commitment, 7),
    "pcs_sumcheck_coefficient_byte": lambda p: _flip(p.pcs._polys, 17),
    "query_record_byte": lambda p: _flip(p.pcs.fri_proof._q, 5 * p.pcs.fri_proof.qbytes + 40),
    "width_header": lambda p: setattr(p.c, "width", p.c.width + 1),
    "degree_header": lambda p: setattr(p.c, "degree", p.c.degree + 1),
    "non_canonical_output": lambda p: ctypes.memmove(p._output, b"\xff" * 16, 16),
    "non_canonical_coefficient": lambda p: ctypes.memmove(p._polys, F.M.to_bytes(16, "little"), 16),
}


@pytest.mark.parametrize("what", sorted(MUTATIONS))
@pytest.mark.parametrize("name", ["pythagorean", "deg5_w7"])
def test_verifier_rejects_altered_proof(name, what):
    mo = S.model(name)
    p = S.pack(mo)
    MUTATIONS[what](p)
    st, digest = _verify(name, mo, p)
    assert st == VERIFY
    assert digest == mo["entry"]  # the transcript is as it was, the root included


@pytest.mark.parametrize("name", ["pythagorean", "deg5_w7"])
def test_verifier_rejects_wrong_sum_and_log_height(name):
    mo = S.model(name)
    p = S.pack(mo)
    st, digest = _verify(name, mo, p, total=(mo["total"] + 1) % F.M)
    assert st == VERIFY and digest == mo["entry"]
    for lh in (mo["log_height"] + 1, mo["log_height"] - 1):
        st, digest = _verify(name, mo, p, log_height=lh)
        assert st == VERIFY and digest == mo["entry"]
    st, digest = _verify(name, mo, p)  # the untouched proof still verifies
    assert st == 0 and digest == mo["digest"]
