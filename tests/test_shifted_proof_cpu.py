"""Next-row constraints on the host: mlh_shift_succ_evaluate against the
explicit sum over the rows, and mlh_system_verify_shifted on the proofs of the
plain-Python model tests/shifted_reference.py -- accepted with the model's
final digest, every alteration rejected with the transcript untouched.  CPU
only; every comparison is exact."""
import ctypes
import random

import pytest

import shifted_reference as SR
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.transcript import Transcript
from oracle import field as F

M = F.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]
VERIFY = _lib.STATUS_CODES["MLH_ERR_VERIFY"]


def _succ(x, y):
    out = (ctypes.c_uint8 * 16)()
    assert D.lib().mlh_shift_succ_evaluate(CS._elems(x), CS._elems(y), len(x), out) == 0
    return D.fe_from_bytes(out)


# ---- mlh_shift_succ_evaluate ----------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_succ_equals_the_sum_over_rows(n):
    rng = random.Random(100 + n)
    for _ in range(4):
        x = [rng.randrange(M) for _ in range(n)]
        y = [rng.randrange(M) for _ in range(n)]
        assert _succ(x, y) == SR.succ_brute(x, y)


def test_succ_on_bits_is_the_successor_relation():
    n = 3

    def point(i):  # bit b of the index <-> point[n - 1 - b]
        return [(i >> (n - 1 - t)) & 1 for t in range(n)]

    for i in range(1 << n):
        for j in range(1 << n):
            assert _succ(point(i), point(j)) == (1 if j == (i + 1) % (1 << n) else 0), (i, j)


def test_succ_argument_errors():
    out = (ctypes.c_uint8 * 16)()
    lib = D.lib()
    assert lib.mlh_shift_succ_evaluate(None, CS._elems([1]), 1, out) == INVALID
    assert lib.mlh_shift_succ_evaluate(CS._elems([1]), CS._elems([1]), 1, None) == INVALID
    assert lib.mlh_shift_succ_evaluate(CS._elems([M]), CS._elems([1]), 1, out) == INVALID
    assert lib.mlh_shift_succ_evaluate(None, None, 0, out) == 0 and D.fe_from_bytes(out) == 1


def test_model_final_check_holds():
    """The model's own proof satisfies the relation the verifier checks, with
    succ as the explicit sum: the model and the protocol agree."""
    mo = SR.model("mixed5")
    lam, W = mo["lam"], mo["width"]
    comb = sum(pow(lam, k, M) * mo["output2"][c] for k, c in enumerate(mo["shifts"])) % M
    claim = sum(pow(lam, k, M) * mo["output"][W + k] for k in range(len(mo["shifts"]))) % M
    from cs_reference import poly_evaluate, to_polynomial

    for pol, r in zip(mo["pols2"], mo["rs2"]):
        claim = poly_evaluate(to_polynomial(pol, claim), r)
    assert mo["succ"] * comb % M == claim


# ---- mlh_system_verify_shifted --------------------------------------------------

def _verify(name, mo, p, shifts=None, n_shifts=None, pre=None, mask=None, total=None,
            log_height=None, wire=None):
    wire0, shifts0 = SR.program(name)
    prog = CS.Program(wire0 if wire is None else wire)
    shifts = shifts0 if shifts is None else shifts
    K = len(shifts) if n_shifts is None else n_shifts
    arr = (ctypes.c_uint32 * max(len(shifts), 1))(*shifts)
    tr = Transcript()
    tr.absorb(mo["seed"])
    assert tr.random() == mo["entry"]
    st = D.lib().mlh_system_verify_shifted(
        prog.h, mo["log_height"] if log_height is None else log_height,
        mo["pre"] if pre is None else pre, mo["mask"] if mask is None else mask, arr, K,
        D.fe_bytes(mo["total"] if total is None else total), D.fe_bytes(mo["column_sum"]),
        ctypes.byref(p.c), tr.h)
    return st, tr.random()


@pytest.mark.parametrize("name", SR.CPU_NAMES)
def test_verifier_accepts_model_proof(name):
    mo = SR.model(name)
    assert SR.program(name)[1] == mo["shifts"]
    st, digest = _verify(name, mo, SR.pack(mo))
    assert st == 0
    assert digest == mo["digest"]


def _flip(buf, i):
    buf[i] ^= 1


MUTATIONS = {
    "output_next_element": lambda p, mo: _flip(p._output, 16 * mo["width"] + 3),
    "output_last_next_element": lambda p, mo: _flip(p._output, len(p._output) - 16),
    "output_real_element": lambda p, mo: _flip(p._output, 5),
    "output2_first": lambda p, mo: _flip(p._output2, 2),
    "output2_source_column": lambda p, mo: _flip(p._output2, 16 * mo["shifts"][0] + 1),
    "output2_last": lambda p, mo: _flip(p._output2, len(p._output2) - 16),
    "shift_polys_first": lambda p, mo: _flip(p._shift_polys, 0),
    "shift_polys_last": lambda p, mo: _flip(p._shift_polys, len(p._shift_polys) - 16),
    "pcs_shift_coefficient": lambda p, mo: _flip(p.pcs_shift[0]._polys, 17 % len(p.pcs_shift[0]._polys)),
    "pcs_shift_last_coefficient": lambda p, mo: _flip(p.pcs_shift[-1]._polys, 1),
    "pcs_shift_query_byte": lambda p, mo: _flip(p.pcs_shift[-1].fri_proof._q,
                                                5 * p.pcs_shift[-1].fri_proof.qbytes + 40),
    "pcs_shift_root": lambda p, mo: _flip(p.c.pcs_shift[0].fri.batch_commitment, 7),
    "pcs_query_byte": lambda p, mo: _flip(p.pcs[0].fri_proof._q, 5 * p.pcs[0].fri_proof.qbytes + 40),
    "sumcheck_coefficient": lambda p, mo: _flip(p._polys, len(p._polys) - 9),
    "n_shifts_header": lambda p, mo: setattr(p.c, "n_shifts", p.c.n_shifts + 1),
    "shift_column_header": lambda p, mo: p.c.shift_columns.__setitem__(0, (p.c.shift_columns[0] + 1) % 3),
    "shift_column_tail_header": lambda p, mo: p.c.shift_columns.__setitem__(31, 1),
    "width_header": lambda p, mo: setattr(p.c, "width", p.c.width + 1),
    "non_canonical_output2": lambda p, mo: ctypes.memmove(p._output2, b"\xff" * 16, 16),
    "non_canonical_next_output": lambda p, mo: ctypes.memmove(
        ctypes.addressof(p._output) + 16 * mo["width"], M.to_bytes(16, "little"), 16),
    "non_canonical_shift_coefficient": lambda p, mo: ctypes.memmove(p._shift_polys,
                                                                     M.to_bytes(16, "little"), 16),
    "null_shift_polys": lambda p, mo: setattr(p.c, "shift_polys", None),
    "null_output2": lambda p, mo: setattr(p.c, "output2", None),
}


@pytest.mark.parametrize("what", sorted(MUTATIONS))
@pytest.mark.parametrize("name", ["fib4", "mixed5"])  # one commitment; two and a sum column
def test_verifier_rejects_altered_proof(name, what):
    mo = SR.model(name)
    p = SR.pack(mo)
    MUTATIONS[what](p, mo)
    st, digest = _verify(name, mo, p)
    assert st == VERIFY
    assert digest == mo["entry"]  # the transcript is as it was, the roots included


def test_verifier_rejects_wrong_shift_list():
    name = "fib4"
    mo = SR.model(name)
    p = SR.pack(mo)
    assert mo["shifts"] == [0, 1]
    st, digest = _verify(name, mo, p, shifts=[1, 0])  # permuted
    assert st == VERIFY and digest == mo["entry"]
    st, digest = _verify(name, mo, p, shifts=[0, 2])  # another column
    assert st == VERIFY and digest == mo["entry"]
    st, digest = _verify(name, mo, p, shifts=[0, 1], n_shifts=1)  # a wrong K: W would be 4
    assert st == VERIFY and digest == mo["entry"]
    st, digest = _verify(name, mo, p, shifts=[0, 1], n_shifts=0)
    assert st == VERIFY and digest == mo["entry"]
    st, digest = _verify(name, mo, p, shifts=[0, 1, 2])  # K = 3: W would be 2
    assert st != 0 and digest == mo["entry"]
    st, digest = _verify(name, mo, p, shifts=[0, 0])  # a duplicate source column
    assert st == INVALID and digest == mo["entry"]
    st, digest = _verify(name, mo, p, shifts=[0, 3])  # out of range
    assert st == INVALID and digest == mo["entry"]
    st, digest = _verify(name, mo, p)  # the untouched proof still verifies
    assert st == 0 and digest == mo["digest"]


def test_verifier_rejects_wrong_public_inputs():
    name = "mixed5"
    mo = SR.model(name)
    p = SR.pack(mo)
    for kw in (dict(pre=1), dict(pre=3), dict(mask=0), dict(mask=mo["mask"] | 1),
               dict(total=(mo["total"] + 1) % M), dict(log_height=4), dict(log_height=6)):
        st, digest = _verify(name, mo, p, **kw)
        assert st == VERIFY and digest == mo["entry"], kw
    st, digest = _verify(name, mo, p, mask=mo["mask"] | (1 << mo["width"]))  # a next column
    assert st == VERIFY and digest == mo["entry"]


@pytest.mark.parametrize("name", ["fib_broken_mid", "fib_broken_wrap"])
def test_verifier_rejects_a_trace_that_breaks_one_step(name):
    """The relation fails at exactly one row -- a step in the middle, or the
    wrap from the last row to row 0 with the selector left open -- and the
    prover claims sum 0 all the same."""
    mo = SR.model(name)
    W, Wx, H = 3, 5, 1 << mo["log_height"]
    E = mo["extension"]
    broken = [i for i in range(H) if any(f(E[i * Wx:(i + 1) * Wx], []) for f in SR.FIB_FNS)]
    assert broken == [6 if name == "fib_broken_mid" else H - 1]
    st, digest = _verify(name, mo, SR.pack(mo))
    assert st == VERIFY and digest == mo["entry"]


def test_satisfied_fibonacci_has_no_broken_row():
    mo = SR.model("fib4")
    E = mo["extension"]
    assert not any(f(E[i * 5:(i + 1) * 5], []) for i in range(16) for f in SR.FIB_FNS)


# ---- the compile step -------------------------------------------------------------

def test_compile_shifted_collects_distinct_columns_in_order():
    from multilinear_amd.constraint_system import compile_program, compile_shifted, nxt, var

    wire, shifts = compile_shifted([nxt(2) * var(0) - nxt(0), nxt(2) + nxt(1)], 3, 0, 2)
    assert shifts == [2, 0, 1]
    assert wire == compile_program([var(3) * var(0) - var(4), var(3) + var(5)], 6, 0, 2)
    wire, shifts = compile_shifted([var(1) * var(0)], 3, 0, 2)
    assert shifts == [] and wire == compile_program([var(1) * var(0)], 3, 0, 2)
    with pytest.raises(ValueError):
        compile_shifted([nxt(3)], 3, 0, 1)
    with pytest.raises(ValueError):
        compile_program([nxt(0)], 3, 0, 1)
    with pytest.raises(ValueError):
        compile_shifted([nxt(j) for j in range(17)], 17, 0, 1)  # 17 + 17 > 32
