"""Plain-Python model of the two-phase system proof (mlh_system_prove_phased /
mlh_system_verify_phased), for tests/test_phased_proof_*.py.  No libmlhip
arithmetic: it composes

  tests/cs_reference.py                   System, SumcheckTables (with its own
                                          partial sum carrying the beta term)
  oracle.transcript                       Transcript
  oracle.batched.BatchedPCSProof.prove    the two openings

in the order of include/mlhip.h: root1, the trace randoms, root2, the row and
constraint challenges, LE16(column_sum) and beta, the sumcheck of

  sum_i [ delta[i] composition(row_i) + beta sum_{j in S} row_i[j] ]
      = sum + beta column_sum,

the opening of columns [0, P) at (rs, output[0:P]) and that of [P, W) at (rs,
output[P:W]).  Above 2^9 rows the C oracle stands in for the Python batched
PCS, started through its `prefix`; the prefix of the second opening is the
first's followed by every byte the first opening absorbs, in the order
system_reference._query_indices replays.
"""
import ctypes
import functools

import cs_cases
import cs_reference as R
import system_reference as S
from oracle import field as F
from oracle import transcript as OT

M = F.M

# name -> (pre_random_columns, sum columns)
LAYOUTS = {
    "lin1": (1, (0,)),                  # L = 1: no fused fold-and-sums pass
    "quad3": (1, (2,)),                 # q = 1
    "pythagorean": (4, ()),             # one phase, no sums: mlh_system_prove
    "deg5_w7": (4, (0, 6)),             # a sum column in each phase; 2 randoms
    "wide32": (31, tuple(range(32))),   # a one-column second commitment
    "cubic4": (2, (3,)),                # several blocks / row pairs per thread; C-oracle route
}
NAMES = ["lin1", "quad3", "pythagorean", "deg5_w7", "wide32", "cubic4"]


def column_mask(cols):
    m = 0
    for j in cols:
        m |= 1 << j
    return m


class SumTables(R.SumcheckTables):
    """SumcheckTables whose partial sum carries beta * sum_{j in S} of the row
    at X = r beside delta * composition."""

    def __init__(self, matrix, width, height, delta, sum_columns, beta):
        super().__init__(matrix, width, height, delta)
        self.sum_columns = tuple(sum_columns)
        self.beta = beta

    def partial_sum(self, composition, r):
        base = super().partial_sum(composition, r)
        if not self.sum_columns:
            return base
        off = self.height >> 1
        w, mat = self.width, self.matrix
        s = (1 - r) % M
        lin = 0
        for i in range(off):
            for j in self.sum_columns:
                lin += s * mat[i * w + j] + r * mat[(i + off) * w + j]
        return (base + self.beta * (lin % M)) % M


def sumcheck(sysm, ot, sum_columns, beta, claim):
    """-> (pols, rs, output): the rounds on `ot` and row 0 of the folded matrix."""
    t = sysm.build_tables()
    tables = SumTables(t.matrix, t.width, t.height, t.delta, sum_columns, beta)
    pols, rs = sysm.compute_sumcheck_polynomials(ot, tables, claim)
    return pols, rs, tables.matrix[:sysm.columns]


def prove(seed, fns, degree, width, randoms, log_height, matrix, pre, sum_columns, total=None,
          column_sum=None, matrix1=None, matrix2=None):
    """-> dict: the proof's parts in host form and the transcript digests.
    matrix1 / matrix2 (optional): the trace as commitment 1 / 2 and its
    opening saw it."""
    P, W = pre, width
    columns = S.columns_of(matrix, W)
    columns1 = S.columns_of(matrix if matrix1 is None else matrix1, W)[:P]
    columns2 = S.columns_of(matrix if matrix2 is None else matrix2, W)[P:]
    root1 = S.batch_root(columns1, log_height)
    root2 = S.batch_root(columns2, log_height) if P < W else None
    ot = OT.Transcript()
    ot.absorb(seed)
    entry = ot.random()
    ot.absorb(root1)                                                       # 1
    trace_randoms = [ot.next_challenge()] * randoms                        # 2
    if root2 is not None:
        ot.absorb(root2)                                                   # 3
    sysm = R.System(ot, fns, degree, W, randoms, log_height, matrix)       # 4
    sysm.challenges.trace = trace_randoms
    delta = [R.mask_evaluate(i, log_height, sysm.challenges.row) for i in range(1 << log_height)]
    if total is None:
        total = sum(d * sysm.evaluate_composition(matrix[i * W:(i + 1) * W])
                    for i, d in enumerate(delta)) % M
    if column_sum is None:
        column_sum = sum(matrix[i * W + j] for i in range(1 << log_height) for j in sum_columns) % M
    beta, prefix = 0, seed + root1 + (root2 or b"")
    if sum_columns:                                                        # 5
        ot.absorb(F.to_bytes(column_sum))
        prefix += F.to_bytes(column_sum)
        beta = ot.next_challenge()
    claim = (total + beta * column_sum) % M
    before_sumcheck = ot.clone()
    pols, rs, output = sumcheck(sysm, ot, sum_columns, beta, claim)        # 6
    after_sumcheck = ot.random()
    coeff_bytes = b"".join(F.to_bytes(c) for p in pols for c in p)
    prefix += coeff_bytes
    openings = []
    pcs1, prefix = S._open(ot, prefix, rs, output[:P], columns1, log_height, openings)  # 7
    pcs = [pcs1]
    if P < W:
        pcs2, prefix = S._open(ot, prefix, rs, output[P:], columns2, log_height, openings)  # 8
        pcs.append(pcs2)
        assert pcs2["batch_commitment"] == root2
    assert pcs1["batch_commitment"] == root1
    digest = ot.random()
    assert digest == pcs[-1]["last_random"]
    return dict(openings=openings,
                seed=seed, entry=entry, root1=root1, root2=root2, sysm=sysm, matrix=matrix,
                columns=columns, total=total, column_sum=column_sum, beta=beta, claim=claim,
                trace_randoms=trace_randoms, before_sumcheck=before_sumcheck, pols=pols, rs=rs,
                output=output, after_sumcheck=after_sumcheck, coeff_bytes=coeff_bytes, pcs=pcs,
                digest=digest, log_height=log_height, width=W, degree=degree, pre=P,
                sum_columns=tuple(sum_columns), mask=column_mask(sum_columns), randoms=randoms)


@functools.lru_cache(maxsize=None)
def model(name):
    """The model's phased proof of a tests/cs_cases.py system under LAYOUTS,
    computed once."""
    P, sc = LAYOUTS[name]
    if name == "pythagorean":
        return prove(b"", cs_cases.PYTHAGOREAN_FNS, 2, 4, 0, 4, cs_cases.pythagorean_matrix(), P, sc,
                     total=0)
    c = S.CASES[name]
    return prove(c.seed, c.fns, c.degree, c.width, c.randoms, c.log_height, c.matrix(), P, sc)


def pack(mo):
    """A model proof as mlh_phased_proof: a multilinear_amd PhasedSystemProof
    (the buffer holder) filled with the model's bytes."""
    from multilinear_amd.constraint_system import PhasedSystemProof

    p = PhasedSystemProof(mo["log_height"], mo["width"], mo["degree"], mo["pre"], mo["mask"])
    ctypes.memmove(p._polys, mo["coeff_bytes"], len(mo["coeff_bytes"]))
    out = b"".join(F.to_bytes(v) for v in mo["output"])
    ctypes.memmove(p._output, out, len(out))
    for i, pcs in enumerate(mo["pcs"]):
        S._fill_pcs(p.pcs[i], p.c.pcs[i], pcs)
    p._sync()
    return p
