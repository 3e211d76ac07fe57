"""Soundness of the host verifiers: the forged proofs of tests/forge_reference.py
(consistent transcript, trees and openings, one lie each) through
mlh_fri_verify, mlh_pcs_verify, mlh_batched_fri_verify, mlh_batched_pcs_verify,
mlh_system_verify and mlh_system_verify_phased.  For every corpus member: the
C verdict is the oracle's, it is the expected one (only the honest member of a
family is accepted), explain() names exactly the targeted check, and a
rejecting system verifier leaves the caller's transcript as it was.  Runs
without a GPU.

c_verdict() / system_status() / phased_status() take the library to call, so
tests/test_verifier_mutants_cpu.py drives its own builds of verify.cpp through
the same code."""
import ctypes

import pytest

import forge_reference as FR
import phased_reference as PR
import system_reference as S
from multilinear_amd import _lib
from oracle import field as F

VERIFY = _lib.STATUS_CODES["MLH_ERR_VERIFY"]


def _fill_fri_struct(proof, log_code):
    """Pack an oracle FriProof into the C struct layout of mlhip.h."""
    from multilinear_amd import _lib as L

    T = log_code - 1
    commit = (ctypes.c_uint8 * (32 * T)).from_buffer_copy(b"".join(proof.commitments))
    qb = L.load().mlh_fri_query_bytes(log_code)
    raw = b""
    for q in proof.queries:
        for value, path in q:
            raw += value + b"".join(s for s, _ in path)
    assert len(raw) == qb * 128
    qbuf = (ctypes.c_uint8 * len(raw)).from_buffer_copy(raw)
    c = L.FriProofC()
    c.log_code = log_code
    c.num_trees = T
    c.num_queries = 128
    c.commitments = ctypes.cast(commit, ctypes.c_void_p)
    c.last_elem[:] = list(F.to_bytes(proof.last_elem))
    c.last_random[:] = list(proof.last_random)
    c.query_indices = None
    c.queries = ctypes.cast(qbuf, ctypes.c_void_p)
    return c, (commit, qbuf)


def _fill_batched(proof, log_code, m):
    """oracle BatchedFriProof -> C layout (mlh_batched_fri_proof)."""
    from multilinear_amd.batched import BatchedFriProof

    p = BatchedFriProof(log_code, m)
    raw = b""
    for (col, bpath), inner in proof.queries:
        raw += b"".join(col) + b"".join(s for s, _ in bpath)
        for value, path in inner:
            raw += value + b"".join(s for s, _ in path)
    assert len(raw) == p.qbytes * 128
    ctypes.memmove(p._q, raw, len(raw))
    if proof.commitments:
        ctypes.memmove(p._commit, b"".join(proof.commitments), 32 * len(proof.commitments))
    p.c.num_trees = len(proof.commitments)
    p.c.num_queries = 128
    p.c.query_indices = None
    p.c.batch_commitment[:] = list(proof.batch_commitment)
    p.c.last_elem[:] = list(F.to_bytes(proof.last_elem))
    p.c.last_random[:] = list(proof.last_random)
    return p


# ---- calling a library's verifiers ----------------------------------------------

def _elems(vals):
    raw = b"".join(int(v).to_bytes(16, "little") for v in vals)
    return (ctypes.c_uint8 * max(16, len(raw))).from_buffer_copy(raw.ljust(16, b"\0"))


class CTranscript:
    """An mlh_transcript of `lib` with `start` absorbed."""

    def __init__(self, lib, start=b""):
        self.lib, h = lib, ctypes.c_void_p()
        assert lib.mlh_transcript_create(ctypes.byref(h)) == 0
        self.h = h.value
        if start:
            buf = (ctypes.c_uint8 * len(start)).from_buffer_copy(start)
            assert lib.mlh_transcript_absorb(self.h, buf, len(start)) == 0

    def random(self):
        out = (ctypes.c_uint8 * 32)()
        assert self.lib.mlh_transcript_random(self.h, out) == 0
        return bytes(out)

    def __del__(self):
        self.lib.mlh_transcript_destroy(self.h)


def _indices(proof):
    idx = FR.opened_indices(proof)
    return (ctypes.c_uint64 * len(idx))(*idx)


def c_verdict(lib, member, indices=False):
    """-> the status of member's proof in `lib`'s verifier of its kind.
    indices: query_indices filled with what the openings' directions spell
    (what the wire decoder hands over); else NULL."""
    pr, kind = member.proof, member.kind
    idx = _indices(pr) if indices else None  # (alive across the call)
    if kind in ("fri", "pcs"):
        fp = pr if kind == "fri" else pr.fri_proof
        c, keep = _fill_fri_struct(fp, len(fp.commitments) + 1)
        if indices:
            c.query_indices = ctypes.cast(idx, ctypes.c_void_p)
        if kind == "fri":
            return lib.mlh_fri_verify(ctypes.byref(c))
        n = len(pr.inputs)
        polys = _elems([x for sp in pr.sumcheck_polynomials for x in sp])
        pc = _lib.PcsProofC()
        pc.fri = c
        pc.sumcheck_polys = ctypes.cast(polys, ctypes.c_void_p)
        tr = CTranscript(lib, member.start)
        return lib.mlh_pcs_verify(ctypes.byref(pc), n, _elems(pr.inputs), _elems([pr.output]), tr.h)
    m, n = member.shape
    p = _fill_batched(pr if kind == "batched_fri" else pr.fri_proof, n + 1, m)
    if indices:
        p.c.query_indices = ctypes.cast(idx, ctypes.c_void_p)
    if kind == "batched_fri":
        return lib.mlh_batched_fri_verify(ctypes.byref(p.c))
    polys = _elems([x for sp in pr.sumcheck_polynomials for x in sp])
    pc = _lib.BatchedPcsProofC()
    pc.fri = p.c
    pc.sumcheck_polys = ctypes.cast(polys, ctypes.c_void_p)
    tr = CTranscript(lib, member.start)
    return lib.mlh_batched_pcs_verify(ctypes.byref(pc), n, _elems(pr.inputs), _elems(pr.outputs), tr.h)


class CProgram:
    def __init__(self, lib, wire):
        self.lib, h = lib, ctypes.c_void_p()
        buf = (ctypes.c_uint8 * len(wire)).from_buffer_copy(bytes(wire))
        assert lib.mlh_cs_program_create(buf, len(wire), ctypes.byref(h)) == 0
        self.h = h.value

    def __del__(self):
        self.lib.mlh_cs_program_destroy(self.h)


def system_status(lib, name, mo, total):
    """-> (status, transcript digest after the call) of mlh_system_verify."""
    prog, tr, p = CProgram(lib, S.program_wire(name)), CTranscript(lib, mo["seed"]), S.pack(mo)
    assert tr.random() == mo["entry"]
    st = lib.mlh_system_verify(prog.h, mo["log_height"], _elems([total]), ctypes.byref(p.c), tr.h)
    return st, tr.random()


def phased_status(lib, name, mo, total, column_sum):
    """-> (status, transcript digest after the call) of mlh_system_verify_phased."""
    prog, tr, p = CProgram(lib, S.program_wire(name)), CTranscript(lib, mo["seed"]), PR.pack(mo)
    assert tr.random() == mo["entry"]
    st = lib.mlh_system_verify_phased(prog.h, mo["log_height"], mo["pre"], mo["mask"], _elems([total]),
                                      _elems([column_sum]), ctypes.byref(p.c), tr.h)
    return st, tr.random()


# ---- FRI / PCS / batched ------------------------------------------------------------

CORPUS = FR.corpus()


def test_corpus_covers_every_family_and_shape():
    kinds = {}
    for m in CORPUS:
        kinds.setdefault(m.kind, set()).add((m.shape, m.lie and m.lie[0]))
    for kind, shapes in (("fri", [(n,) for n in FR.FRI_LOGS]), ("pcs", [(n,) for n in FR.FRI_LOGS]),
                         ("batched_fri", FR.BATCHED_SHAPES), ("batched_pcs", FR.BATCHED_SHAPES)):
        for shape in shapes:
            fams = {f for s, f in kinds[kind] if s == shape}
            assert {None, "wrong_index", "wrong_directions", "wrong_root", "stale_last_random",
                    "noncanonical"} <= fams
            if kind.endswith("fri"):
                assert {"wrong_challenge", "last_elem"} <= fams
            else:
                assert {"wrong_claim", "wrong_poly", "other_polynomial"} <= fams
    assert ("batch_column" in {f for s, f in kinds["batched_fri"] if s == (2, 1)})  # num_trees == 0


@pytest.mark.parametrize("kind", ["fri", "pcs", "batched_fri", "batched_pcs"])
def test_honest_forger_is_the_oracle_prover(kind):
    """lie=None: byte for byte what the oracle's prove() returns."""
    from oracle import batched as OB
    from oracle import fri as OF
    from oracle import pcs as OP
    from oracle import transcript as OT

    for m in (m for m in CORPUS if m.kind == kind and m.lie is None):
        if kind == "fri":
            (ln,) = m.shape
            gp = F.pow_2_generator_powers(ln + 1)
            want = OF.FriProof.prove(OF.reed_solomon(FR.rand_vals(100 + ln, 1 << ln), gp[1]), gp,
                                     OT.Transcript())
        elif kind == "pcs":
            (n,) = m.shape
            pts, ev = FR.rand_vals(200 + n, n), FR.rand_vals(300 + n, 1 << n)
            want = OP.PCSProof.prove(pts, FR._mle(ev, pts), ev, m.transcript())
        elif kind == "batched_fri":
            mm, ln = m.shape
            gp = F.pow_2_generator_powers(ln + 1)
            codes = [OF.reed_solomon(FR.rand_vals(400 + 10 * ln + j, 1 << ln), gp[1]) for j in range(mm)]
            want = OB.BatchedFriProof.prove(codes, gp, OT.Transcript())
        else:
            mm, n = m.shape
            pts = FR.rand_vals(500 + n, n)
            polys = [FR.rand_vals(600 + 10 * n + j, 1 << n) for j in range(mm)]
            want = OB.BatchedPCSProof.prove(pts, [FR._mle(p, pts) for p in polys], polys, m.transcript())
        assert FR.proof_bytes(m.proof) == FR.proof_bytes(want), m.id


def test_flat_records_round_trip():
    """fri_from_flat / batched_from_flat (which read the device's proofs in
    the GPU tests) invert the struct fillers' flattening."""
    for m in CORPUS:
        if m.lie and m.lie[0] in ("wrong_index", "wrong_directions"):
            continue  # their directions are not what the drawn index spells
        fp = getattr(m.proof, "fri_proof", m.proof)
        idx = FR.opened_indices(m.proof)
        if m.kind in ("fri", "pcs"):
            raw = b"".join(v + b"".join(s for s, _ in p) for q in fp.queries for v, p in q)
            back = FR.fri_from_flat(fp.commitments, raw, idx, fp.last_elem, fp.last_random)
        else:
            back = FR.batched_from_flat(fp.batch_commitment, fp.commitments, m.shape[0],
                                        S._flat_queries(fp.queries), idx, fp.last_elem, fp.last_random)
        assert FR.proof_bytes(back) == FR.proof_bytes(fp), m.id


@pytest.mark.parametrize("member", CORPUS, ids=[m.id for m in CORPUS])
def test_forgery_fails_exactly_the_targeted_check(member):
    lib = _lib.load()
    got = member.explain()
    oracle = member.oracle()
    assert oracle == (not got)                   # explain's verdict is the oracle's
    assert oracle == (member.lie is None)        # only the honest member is accepted
    assert member.matches(got), (got, member.expect)
    st = c_verdict(lib, member, indices=True)    # as decoded from the wire: indices present
    assert st == (0 if oracle else VERIFY)
    # query_indices NULL: the struct carries no directions, so K5 cannot be seen
    st = c_verdict(lib, member)
    assert st == (0 if not (got - {"K5"}) else VERIFY)


# ---- public inputs >= M ---------------------------------------------------------------

def test_noncanonical_public_inputs_keep_their_status():
    """Proof elements >= M are MLH_ERR_VERIFY (the K11 members above).  Public
    inputs are the caller's and keep the status they had before that rule:
    mlh_pcs_verify does not absorb `output` and computes mod M, so output + M
    is the same claim (accepted); inputs[0] + M breaks Delta::evaluate's
    1 - a (MLH_ERR_VERIFY); mlh_batched_pcs_verify absorbs the bytes of both,
    the transcript diverges (MLH_ERR_VERIFY); the system verifiers answer
    MLH_ERR_VERIFY to a sum >= M and leave the transcript alone."""
    lib = _lib.load()
    pts, ev = [2, 3, 5], FR.small_vals(8)
    m = FR.Member("pcs", (3,), None, None, set(), b"public")
    m.proof = FR.forge_pcs(pts, FR._mle(ev, pts), ev, m.transcript())
    assert m.proof.output < FR.NC and c_verdict(lib, m) == 0
    m.proof.output += F.M
    assert c_verdict(lib, m) == 0
    m.proof.output -= F.M
    m.proof.inputs = [2 + F.M, 3, 5]
    assert c_verdict(lib, m) == VERIFY
    polys = [FR.small_vals(2, j) for j in range(2)]
    b = FR.Member("batched_pcs", (2, 1), None, None, set(), b"public")
    b.proof = FR.forge_batched_pcs([7], [FR._mle(p, [7]) for p in polys], polys, b.transcript())
    assert b.proof.outputs[0] < FR.NC and c_verdict(lib, b) == 0
    b.proof.outputs[0] += F.M
    assert c_verdict(lib, b) == VERIFY
    b.proof.outputs[0] -= F.M
    b.proof.inputs[0] += F.M
    assert c_verdict(lib, b) == VERIFY
    mo = S.model("lin1")
    st, digest = system_status(lib, "lin1", mo, 2**128 - 1)
    assert st == VERIFY and digest == mo["entry"]


# ---- system level -----------------------------------------------------------------------

SYSTEM_MEMBERS = [(n, l) for n in FR.SYSTEM_NAMES for l in FR.SYSTEM_LIES]
PHASED_MEMBERS = [(n, l) for n in FR.PHASED_NAMES for l in FR.PHASED_LIES[n]]


@pytest.mark.parametrize("name,lie", SYSTEM_MEMBERS)
def test_system_forgery_fails_exactly_the_targeted_check(name, lie):
    mo, total, expect = FR.system_forgery(name, lie)
    got = FR.explain_system(mo, total)
    assert got == expect
    assert FR.system_verdict(mo, total) == (not got) == (lie is None)
    st, digest = system_status(_lib.load(), name, mo, total)
    if lie is None:
        assert st == 0 and digest == mo["digest"]
    else:
        assert st == VERIFY and digest == mo["entry"]  # the caller's transcript is untouched


@pytest.mark.parametrize("name,lie", PHASED_MEMBERS)
def test_phased_forgery_fails_exactly_the_targeted_check(name, lie):
    mo, total, column_sum, expect = FR.phased_forgery(name, lie)
    got = FR.explain_system(mo, total, column_sum)
    assert got == expect
    assert FR.system_verdict(mo, total, column_sum) == (not got) == (lie is None)
    st, digest = phased_status(_lib.load(), name, mo, total, column_sum)
    if lie is None:
        assert st == 0 and digest == mo["digest"]
    else:
        assert st == VERIFY and digest == mo["entry"]
