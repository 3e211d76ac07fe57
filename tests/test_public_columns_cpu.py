"""Public columns on the host: the spec decoder, mlh_public_columns_evaluate
against the explicit sum over the rows, and mlh_system_verify_public on the
proofs of the plain-Python model tests/public_reference.py -- accepted with the
model's final digest, every alteration rejected with the transcript untouched.
CPU only; every comparison is exact."""
import ctypes
import hashlib
import random
import struct

import pytest

import public_reference as PUB
import shifted_reference as SR
import test_shifted_proof_cpu as TS
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.transcript import Transcript
from oracle import field as F

M = F.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]
VERIFY = _lib.STATUS_CODES["MLH_ERR_VERIFY"]


def _create(wire):
    """-> (status, handle or None)."""
    h = ctypes.c_void_p()
    buf = (ctypes.c_uint8 * max(len(wire), 1)).from_buffer_copy(wire or b"\0")
    st = D.lib().mlh_public_columns_create(buf, len(wire), ctypes.byref(h))
    return st, h.value


class Spec:
    """A handle made from raw wire bytes."""

    def __init__(self, wire):
        st, self.h = _create(wire)
        assert st == 0

    def __del__(self):
        D.lib().mlh_public_columns_destroy(self.h)

    def evaluate(self, L, point):
        out = (ctypes.c_uint8 * (16 * D.lib().mlh_public_columns_count(self.h)))()
        st = D.lib().mlh_public_columns_evaluate(self.h, L, CS._elems(point), out)
        return st, CS._split(out, len(out) // 16)


# ---- mlh_public_columns_evaluate ------------------------------------------------------

def _every_kind(L, rng):
    H = 1 << L
    r = lambda: rng.randrange(M)  # noqa: E731
    return [("const", r()), ("first",), ("last",), ("row",), ("periodic", [r()]),
            ("periodic", [r(), r()]), ("periodic", [r() for _ in range(H)]),
            ("sparse", {0: r(), H - 1: r()} if H > 1 else {0: r()}), ("sparse", {H - 1: r()}),
            ("sparse", {i: r() for i in range(0, H, 3)})]


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 6])
def test_evaluate_equals_the_sum_over_rows(L):
    rng = random.Random(200 + L)
    ds = _every_kind(L, rng)
    spec = Spec(PUB.wire(ds))
    for _ in range(3):
        point = [rng.randrange(M) for _ in range(L)]
        st, got = spec.evaluate(L, point)
        assert st == 0
        assert got == PUB.public_at(ds, L, point)


def test_evaluate_on_bits_is_the_column():
    L, H = 3, 8
    ds = _every_kind(L, random.Random(7))
    spec = Spec(PUB.wire(ds))
    cols = [PUB.column(d, H) for d in ds]
    for i in range(H):  # bit b of the index <-> point[L - 1 - b]
        st, got = spec.evaluate(L, [(i >> (L - 1 - t)) & 1 for t in range(L)])
        assert st == 0 and got == [c[i] for c in cols], i


def test_one_row_is_both_first_and_last():
    spec = Spec(PUB.wire([("first",), ("last",), ("row",), ("periodic", [5]), ("sparse", {0: 9})]))
    assert spec.evaluate(0, []) == (0, [1, 1, 0, 5, 9])


def test_builder_encodes_the_wire_and_evaluates():
    ds = _every_kind(4, random.Random(8))
    pc = PUB.builder(ds)
    assert pc.wire == PUB.wire(ds) and len(pc) == len(ds)
    assert pc.digest == hashlib.sha256(pc.wire).digest()
    point = [3, 5, 7, 11]
    assert pc.evaluate(point) == PUB.public_at(ds, 4, point)
    with pytest.raises(ValueError):
        CS.PublicColumns().periodic([1, 2, 3])


def test_digest_is_sha256_of_the_wire():
    w = PUB.wire(PUB.descs("pmixed5"))
    spec = Spec(w)
    out = (ctypes.c_uint8 * 32)()
    assert D.lib().mlh_public_columns_digest(spec.h, out) == 0
    assert bytes(out) == hashlib.sha256(w).digest()
    assert D.lib().mlh_public_columns_count(spec.h) == 3
    assert D.lib().mlh_public_columns_count(None) == 0
    assert D.lib().mlh_public_columns_digest(None, out) == INVALID
    assert D.lib().mlh_public_columns_digest(spec.h, None) == INVALID


def test_height_dependent_conditions():
    per = Spec(PUB.wire([("periodic", [1, 2, 3, 4])]))  # k = 2
    assert per.evaluate(1, [1])[0] == INVALID
    assert per.evaluate(2, [1, 2])[0] == 0
    sp = Spec(PUB.wire([("sparse", {0: 1, 4: 2})]))
    assert sp.evaluate(2, [1, 2])[0] == INVALID  # row 4 >= 2^2
    assert sp.evaluate(3, [1, 2, 3])[0] == 0
    assert sp.evaluate(3, [1, M, 3])[0] == INVALID  # non-canonical point
    out = (ctypes.c_uint8 * 16)()
    assert D.lib().mlh_public_columns_evaluate(sp.h, 3, None, out) == INVALID
    assert D.lib().mlh_public_columns_evaluate(sp.h, 3, CS._elems([1, 2, 3]), None) == INVALID
    assert D.lib().mlh_public_columns_evaluate(None, 3, CS._elems([1, 2, 3]), out) == INVALID
    assert D.lib().mlh_public_columns_evaluate(sp.h, 33, CS._elems([1] * 33), out) == INVALID


# ---- the decoder ------------------------------------------------------------------------

def _col(kind, arg, payload=b""):
    return struct.pack("<2I", kind, arg) + payload


def _spec(*cols, count=None, reserved=0):
    return struct.pack("<2I", len(cols) if count is None else count, reserved) + b"".join(cols)


E1, BIG = F.to_bytes(1), M.to_bytes(16, "little")
REJECTED = {
    "empty": b"",
    "no_columns": _spec(),
    "seventeen_columns": _spec(*[_col(1, 0)] * 17),
    "unknown_kind": _spec(_col(6, 0)),
    "unknown_kind_large": _spec(_col(0xFFFFFFFF, 0)),
    "reserved_word": _spec(_col(1, 0), reserved=1),
    "const_arg": _spec(_col(0, 1, E1)),
    "first_arg": _spec(_col(1, 1)),
    "last_arg": _spec(_col(2, 7)),
    "row_arg": _spec(_col(3, 1)),
    "periodic_arg_17": _spec(_col(4, 17, E1 * (1 << 17))),
    "sparse_arg_0": _spec(_col(5, 0)),
    "sparse_arg_4097": _spec(_col(5, 4097, b"".join(struct.pack("<Q", r) + E1 for r in range(4097)))),
    "non_canonical_const": _spec(_col(0, 0, BIG)),
    "non_canonical_periodic": _spec(_col(4, 1, E1 + BIG)),
    "non_canonical_sparse": _spec(_col(5, 1, struct.pack("<Q", 3) + b"\xff" * 16)),
    "sparse_unsorted": _spec(_col(5, 2, struct.pack("<Q", 5) + E1 + struct.pack("<Q", 2) + E1)),
    "sparse_repeated": _spec(_col(5, 2, struct.pack("<Q", 5) + E1 + struct.pack("<Q", 5) + E1)),
    "short_header": struct.pack("<I", 1),
    "short_column_header": _spec(_col(1, 0))[:-1],
    "short_const": _spec(_col(0, 0, E1))[:-1],
    "short_periodic": _spec(_col(4, 2, E1 * 3)),
    "short_sparse": _spec(_col(5, 2, struct.pack("<Q", 5) + E1)),
    "missing_column": _spec(_col(1, 0), count=2),
    "trailing_byte": _spec(_col(1, 0)) + b"\0",
    "trailing_column": _spec(_col(1, 0), _col(2, 0), count=1),
}


@pytest.mark.parametrize("what", sorted(REJECTED))
def test_decoder_rejects(what):
    st, h = _create(REJECTED[what])
    assert st == INVALID and h is None


def test_decoder_accepts_the_limits():
    w = _spec(*[_col(4, 16, E1 * (1 << 16))] + [_col(5, 4096, b"".join(
        struct.pack("<Q", 3 * r) + E1 for r in range(4096)))] + [_col(1, 0)] * 14)
    st, h = _create(w)
    assert st == 0 and D.lib().mlh_public_columns_count(h) == 16
    D.lib().mlh_public_columns_destroy(h)
    assert _create(_spec(_col(4, 0, E1)))[0] == 0
    h = ctypes.c_void_p()
    assert D.lib().mlh_public_columns_create(None, 8, ctypes.byref(h)) == INVALID
    assert D.lib().mlh_public_columns_create((ctypes.c_uint8 * 16)(), 16, None) == INVALID


# ---- mlh_system_verify_public -------------------------------------------------------------

def _verify(name, mo, p, spec_wire="model", **kw):
    wire0, shifts0 = PUB.program(name)
    prog = CS.Program(kw.get("wire", wire0))
    shifts = kw.get("shifts", shifts0)
    arr = (ctypes.c_uint32 * max(len(shifts), 1))(*shifts)
    spec = None if spec_wire is None else Spec(mo["wire"] if spec_wire == "model" else spec_wire)
    tr = Transcript()
    tr.absorb(mo["seed"])
    assert tr.random() == mo["entry"]
    st = D.lib().mlh_system_verify_public(
        prog.h, kw.get("log_height", mo["log_height"]), kw.get("pre", mo["pre"]),
        kw.get("mask", mo["mask"]), arr, kw.get("n_shifts", len(shifts)), spec.h if spec else None,
        D.fe_bytes(kw.get("total", mo["total"])), D.fe_bytes(mo["column_sum"]), ctypes.byref(p.c), tr.h)
    return st, tr.random()


@pytest.mark.parametrize("name", PUB.CPU_NAMES)
def test_verifier_accepts_model_proof(name):
    mo = PUB.model(name)
    assert PUB.program(name)[1] == mo["shifts"]
    # the model's own check: the public part of both outputs is the sum over the rows
    C, W, L = mo["committed"], mo["width"], mo["log_height"]
    assert mo["output"][C:W] == PUB.public_at(mo["descs"], L, mo["rs"])
    assert mo["output2"][C:W] == PUB.public_at(mo["descs"], L, mo["rs2"])
    st, digest = _verify(name, mo, PUB.pack(mo))
    assert st == 0
    assert digest == mo["digest"]


def test_satisfied_statement_has_no_broken_row():
    mo = PUB.model("pfib4")
    E = mo["extension"]
    assert not any(f(E[i * 7:(i + 1) * 7], []) for i in range(16) for f in PUB.PFIB_FNS)
    bad = PUB.model("pfib4_wrong_start")["extension"]
    assert [i for i in range(16) if any(f(bad[i * 7:(i + 1) * 7], []) for f in PUB.PFIB_FNS)] == [0]


@pytest.mark.parametrize("name", ["pfib4", "pmixed5"])
def test_verifier_rejects_each_altered_public_element(name):
    """Every public element of output and of output2, read by a constraint or
    not, is bound to the spec."""
    mo = PUB.model(name)
    C, W = mo["committed"], mo["width"]
    for buf in ("_output", "_output2"):
        for j in range(C, W):
            p = PUB.pack(mo)
            getattr(p, buf)[16 * j] ^= 1
            st, digest = _verify(name, mo, p)
            assert st == VERIFY and digest == mo["entry"], (buf, j)


def _with_sparse_value_changed(ds):
    out = []
    for d in ds:
        if d[0] == "sparse":
            rows = dict(d[1])
            last = max(rows)
            rows[last] = (rows[last] + 1) % M
            d = ("sparse", rows)
        out.append(d)
    return out


def test_verifier_rejects_another_spec():
    name = "pfib4"
    mo = PUB.model(name)
    p = PUB.pack(mo)
    ds = mo["descs"]
    wrong_input = PUB.wire(_with_sparse_value_changed(ds))  # the wrong public input
    assert wrong_input != mo["wire"]
    swapped = PUB.wire([ds[1], ds[0], ds[2]])  # FIRST and LAST swapped
    for w in (wrong_input, swapped):
        st, digest = _verify(name, mo, p, spec_wire=w)
        assert st == VERIFY and digest == mo["entry"]
    st, digest = _verify(name, mo, p, spec_wire=None)  # the same proof without a spec
    assert st == VERIFY and digest == mo["entry"]
    st, digest = _verify("pmixed5", PUB.model("pmixed5"), PUB.pack(PUB.model("pmixed5")),
                         spec_wire=None)
    assert st == VERIFY and digest == PUB.model("pmixed5")["entry"]
    st, digest = _verify(name, mo, p)  # the untouched proof and spec still verify
    assert st == 0 and digest == mo["digest"]


def test_verifier_refuses_a_spec_that_does_not_fit():
    name = "pfib4"
    mo = PUB.model(name)
    p = PUB.pack(mo)
    tall = PUB.wire([("first",), ("last",), ("sparse", {0: 1, 16: 2})])  # row 16 of 16
    st, digest = _verify(name, mo, p, spec_wire=tall)
    assert st == INVALID and digest == mo["entry"]
    period = PUB.wire([("first",), ("last",), ("periodic", list(range(32)))])
    st, digest = _verify(name, mo, p, spec_wire=period)
    assert st == INVALID and digest == mo["entry"]
    wide = PUB.wire([("first",)] * 5)  # F = W
    st, digest = _verify(name, mo, p, spec_wire=wide)
    assert st == INVALID and digest == mo["entry"]
    four = PUB.wire([("first",)] * 4)  # F = 4: P = 2 > W - F = 1
    st, digest = _verify(name, mo, p, spec_wire=four)
    assert st == VERIFY and digest == mo["entry"]


@pytest.mark.parametrize("what", sorted(TS.MUTATIONS))
@pytest.mark.parametrize("name", ["pfib4", "pmixed5"])  # one commitment; two and a sum column
def test_verifier_rejects_altered_proof(name, what):
    """The shifted proof's mutations, on the proof with public columns."""
    mo = PUB.model(name)
    p = PUB.pack(mo)
    TS.MUTATIONS[what](p, mo)
    st, digest = _verify(name, mo, p)
    assert st == VERIFY
    assert digest == mo["entry"]


def test_verifier_rejects_wrong_public_inputs():
    name = "pmixed5"
    mo = PUB.model(name)
    p = PUB.pack(mo)
    for kw in (dict(pre=1), dict(pre=3), dict(mask=0), dict(mask=mo["mask"] | 1),
               dict(total=(mo["total"] + 1) % M), dict(log_height=4), dict(log_height=6),
               dict(shifts=[4]), dict(mask=mo["mask"] | (1 << mo["width"]))):
        st, digest = _verify(name, mo, p, **kw)
        assert st == VERIFY and digest == mo["entry"], kw


def test_wrong_start_is_rejected():
    """A trace started from a != io[0]: the model's proof of it does not verify."""
    mo = PUB.model("pfib4_wrong_start")
    st, digest = _verify("pfib4", mo, PUB.pack(mo))
    assert st == VERIFY and digest == mo["entry"]


@pytest.mark.parametrize("name", SR.CPU_NAMES)
def test_no_spec_accepts_the_shifted_models_proofs(name):
    """F = 0: mlh_system_verify_public is mlh_system_verify_shifted."""
    mo = SR.model(name)
    wire, shifts = SR.program(name)
    prog = CS.Program(wire)
    tr = Transcript()
    tr.absorb(mo["seed"])
    st = D.lib().mlh_system_verify_public(
        prog.h, mo["log_height"], mo["pre"], mo["mask"],
        (ctypes.c_uint32 * max(len(shifts), 1))(*shifts), len(shifts), None, D.fe_bytes(mo["total"]),
        D.fe_bytes(mo["column_sum"]), ctypes.byref(SR.pack(mo).c), tr.h)
    assert st == 0 and tr.random() == mo["digest"]
