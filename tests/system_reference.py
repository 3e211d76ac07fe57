"""Plain-Python model of the system proof (mlh_system_prove / mlh_system_verify),
for tests/test_system_proof_*.py.  No libmlhip arithmetic: it composes

  tests/cs_reference.py                   System, ChallengeSet, the sumcheck
  oracle.transcript                       Transcript
  oracle.batched.BatchedPCSProof.prove    the opening (batched_pcs.rs:127-180)

in the fixed order: absorb the trace root (system.rs:62-63), ChallengeSet::new
(system.rs:131-146), the constraint sumcheck with delta = eq(row)
(sumcheck.rs:40-53), BatchedPCSProof::prove(inputs = rs, outputs = output).
The root -- the batch commitment, which does not depend on the transcript --
comes from a batched prove on a scratch transcript (the C oracle's), and is
checked against the batch commitment of the proof itself.  Above 2^9 rows the
C oracle stands in for the Python batched PCS, started from the same
transcript state through its `prefix` (a state is a function of the absorbed
bytes): seed, root, every sumcheck coefficient.

pack() lays a model proof out as mlh_system_proof (the pattern of
tests/test_capi.py::test_host_batched_pcs_verifier_accepts_oracle_proof).
"""
import ctypes
import functools

import numpy as np

import cs_cases
import cs_reference as R
from oracle import batched as OB
from oracle import coracle as OC
from oracle import field as F
from oracle import transcript as OT
from oracle.fri import query_index

M = F.M
PY_MAX_LOG = 9  # the Python batched PCS up to here, the C oracle above


def _limbs(values):
    return np.frombuffer(b"".join(int(v).to_bytes(16, "little") for v in values),
                         dtype=np.uint32).reshape(-1, 4).copy()


def columns_of(matrix, width):
    """The trace's column MLEs (what mlh_trace_columns writes, as lists)."""
    return [matrix[j::width] for j in range(width)]


def batch_root(columns, log_height):
    """The batch commitment of the columns: a batched PCS prove on a scratch
    transcript; claim and transcript do not enter the batch layer."""
    flat = [v for c in columns for v in c]
    pr = OC.pcs_prove_par(_limbs(flat), log_height, [0] * log_height, [0] * len(columns),
                          batched=True)
    assert pr["rc"] == 0
    return pr["batch_root"]


def _query_indices(pr, tr):
    """The indices BatchedPCSProof::prove drew (batched_pcs.rs:166-172), by
    the verifier's replay (:186-250) on `tr`, the state before the prove."""
    fp = pr.fri_proof
    for x in pr.inputs:
        tr.absorb(F.to_bytes(x))
    for y in pr.outputs:
        tr.absorb(F.to_bytes(y))
    for i, poly in enumerate(pr.sumcheck_polynomials):
        if i == 0:
            tr.absorb(fp.batch_commitment)
            tr.absorb(F.to_bytes(tr.next_challenge()))
        else:
            tr.absorb(fp.commitments[i - 1])
        for c in poly:
            tr.absorb(F.to_bytes(c))
    tr.absorb(F.to_bytes(fp.last_elem))
    domain = 1 << (len(fp.commitments) + 1 + OB.LOG_BLOWUP)
    out = []
    for _ in range(OB.NUM_QUERIES):
        idx = query_index(tr, domain)
        out.append(idx)
        tr.absorb(idx.to_bytes(8, "little"))
    return out


def _flat_queries(queries):
    raw = b""
    for (col, bpath), inner in queries:
        raw += b"".join(col) + b"".join(s for s, _ in bpath)
        for value, path in inner:
            raw += value + b"".join(s for s, _ in path)
    return raw


def _opening_bytes(tr, inputs, outputs, pcs):
    """Replays an opening on `tr` (the state before it) and returns every byte
    it absorbs, in order (batched_pcs.rs:186-250 as _query_indices)."""
    out = []

    def absorb(b):
        tr.absorb(b)
        out.append(b)

    for x in inputs:
        absorb(F.to_bytes(x))
    for y in outputs:
        absorb(F.to_bytes(y))
    for i, poly in enumerate(pcs["polys"]):
        if i == 0:
            absorb(pcs["batch_commitment"])
            absorb(F.to_bytes(tr.next_challenge()))
        else:
            absorb(pcs["commitments"][i - 1])
        for c in poly:
            absorb(F.to_bytes(c))
    absorb(F.to_bytes(pcs["last_elem"]))
    domain = 1 << (len(pcs["commitments"]) + 1 + OB.LOG_BLOWUP)
    for want in pcs["indices"]:
        idx = query_index(tr, domain)
        assert idx == want
        absorb(idx.to_bytes(8, "little"))
    assert tr.random() == pcs["last_random"]
    return b"".join(out)


def _open(ot, prefix, rs, outputs, columns, log_height, keep=None):
    """One BatchedPCSProof::prove on `ot` (advanced past it) -> (the proof's
    parts, the prefix of whatever follows).  keep (optional list): receives
    the oracle's proof object where the Python batched PCS made it."""
    if log_height <= PY_MAX_LOG:
        before = ot.clone()
        pr = OB.BatchedPCSProof.prove(rs, outputs, columns, ot)
        if keep is not None:
            keep.append(pr)
        fp = pr.fri_proof
        pcs = dict(batch_commitment=fp.batch_commitment, commitments=list(fp.commitments),
                   polys=[tuple(p) for p in pr.sumcheck_polynomials], last_elem=fp.last_elem,
                   last_random=fp.last_random, indices=_query_indices(pr, before),
                   queries=_flat_queries(fp.queries))
        return pcs, None
    flat = [v for c in columns for v in c]
    cp = OC.pcs_prove_par(_limbs(flat), log_height, rs, outputs, batched=True, prefix=prefix)
    assert cp["rc"] == 0
    pcs = dict(batch_commitment=cp["batch_root"], commitments=cp["roots"], polys=cp["polys"],
               last_elem=cp["last_elem"], last_random=cp["last_random"], indices=cp["indices"],
               queries=cp["queries"])
    return pcs, prefix + _opening_bytes(ot, rs, outputs, pcs)


def prove(seed, fns, degree, width, randoms, log_height, matrix, total=None, opening_matrix=None):
    """-> dict: the proof's parts in host form and the transcript digests.
    opening_matrix (optional): the trace the commitment and the opening see
    (tests/forge_reference.py); sumcheck and output stay `matrix`'s."""
    columns = columns_of(matrix if opening_matrix is None else opening_matrix, width)
    root = batch_root(columns, log_height)
    ot = OT.Transcript()
    ot.absorb(seed)
    entry = ot.random()
    ot.absorb(root)                                                       # 1
    sysm = R.System(ot, fns, degree, width, randoms, log_height, matrix)  # 2
    tables = sysm.build_tables()
    if total is None:
        total = sum(d * sysm.evaluate_composition(matrix[i * width:(i + 1) * width])
                    for i, d in enumerate(tables.delta)) % M
    pols, rs = sysm.compute_sumcheck_polynomials(ot, tables, total)       # 3
    output = tables.matrix[:width]
    after_sumcheck = ot.random()
    coeff_bytes = b"".join(F.to_bytes(c) for p in pols for c in p)
    openings = []
    pcs, _ = _open(ot, seed + root + coeff_bytes, rs, output, columns, log_height, openings)  # 4
    digest = ot.random()
    assert pcs["batch_commitment"] == root
    return dict(seed=seed, entry=entry, root=root, sysm=sysm, matrix=matrix, columns=columns,
                total=total, pols=pols, rs=rs, output=output, after_sumcheck=after_sumcheck,
                coeff_bytes=coeff_bytes, pcs=pcs, digest=digest, log_height=log_height, width=width,
                degree=degree, openings=openings)


CASES = {c.name: c for c in cs_cases.cases()}
NAMES = ["pythagorean"] + sorted(CASES, key=lambda n: CASES[n].log_height)


def program_wire(name):
    if name == "pythagorean":
        from multilinear_amd.constraint_system import compile_program

        return compile_program(cs_cases.pythagorean_exprs(), 4, 0, 2)
    return CASES[name].wire


@functools.lru_cache(maxsize=None)
def model(name):
    """The model's proof of a tests/cs_cases.py system, computed once.
    pythagorean: the reference's own test system (sumcheck.rs:305-365), 2^4 x 4
    on a clean transcript, sum 0; the others: random unsatisfied traces, a
    seeded transcript, the true sum."""
    if name == "pythagorean":
        return prove(b"", cs_cases.PYTHAGOREAN_FNS, 2, 4, 0, 4, cs_cases.pythagorean_matrix(), 0)
    c = CASES[name]
    return prove(c.seed, c.fns, c.degree, c.width, c.randoms, c.log_height, c.matrix())


def _fill_pcs(holder, c_pcs, pcs):
    """The model's opening into a multilinear_amd BatchedPCSProof's buffers
    and the mlh_batched_pcs_proof struct `c_pcs` that points at them."""
    fp = holder.fri_proof
    assert len(pcs["queries"]) == fp.qbytes * OB.NUM_QUERIES
    ctypes.memmove(fp._q, pcs["queries"], len(pcs["queries"]))
    if pcs["commitments"]:
        ctypes.memmove(fp._commit, b"".join(pcs["commitments"]), 32 * len(pcs["commitments"]))
    raw = b"".join(F.to_bytes(a) + F.to_bytes(b) for a, b in pcs["polys"])
    ctypes.memmove(holder._polys, raw, len(raw))
    f = c_pcs.fri
    f.num_trees = len(pcs["commitments"])
    f.num_queries = OB.NUM_QUERIES
    f.query_indices = None
    f.batch_commitment[:] = list(pcs["batch_commitment"])
    f.last_elem[:] = list(F.to_bytes(pcs["last_elem"]))
    f.last_random[:] = list(pcs["last_random"])


def pack(mo):
    """A model proof as mlh_system_proof: a multilinear_amd SystemProof (the
    buffer holder) filled with the model's bytes."""
    from multilinear_amd.constraint_system import SystemProof

    L, W, pcs = mo["log_height"], mo["width"], mo["pcs"]
    p = SystemProof(L, W, mo["degree"])
    ctypes.memmove(p._polys, mo["coeff_bytes"], len(mo["coeff_bytes"]))
    out = b"".join(F.to_bytes(v) for v in mo["output"])
    ctypes.memmove(p._output, out, len(out))
    _fill_pcs(p.pcs, p.c.pcs, pcs)
    p._sync()
    return p
