"""Plain-Python model of the reference's constraint-system sumcheck, for the
tests of the device path (tests/test_cs_sumcheck_*.py).  A restatement of

  constraint_system/sumcheck.rs:21-256    System::{build_tables,
      compute_sumcheck_polynomials, verify_sumcheck_debug,
      verify_with_evaluations}, SumcheckTables::{compute_sumcheck_polynomial(s),
      partial_sum, fold}, SumcheckPolynomial::to_polynomial (:269-276)
  constraint_system/system.rs:74-146      System::new, ChallengeSet::new
  constraint_system/evaluation.rs:4-29,75-91   evaluate_composition,
      evaluate_delta, ConstraintSet::evaluate, Delta::evaluate (and Mask /
      Trace::evaluate, :31-73)
  polynomials.rs:9-14,51-98               Polynomial::evaluate,
      PolynomialEvals::interpolate (the Lagrange loop), poly_mul

over oracle.field / oracle.transcript.  Constraints are Python callables
``f(var, rand) -> int`` (the reference's Expr closures), so the model shares
nothing with the constraint-program bytecode it is compared against.
"""
from oracle import field as F

M = F.M


# ---- polynomials.rs ----------------------------------------------------------

def poly_mul(a, b):  # polynomials.rs:90-98
    out = [0] * (len(a) + len(b) - 1)
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            out[i + j] = (out[i + j] + ai * bj) % M
    return out


def interpolate(evals):  # polynomials.rs:51-87
    n = len(evals)
    coeffs = [0] * n
    for j, yj in enumerate(evals):
        lj = [1]
        xj = F.from_i64(j)
        denom = 1
        for m in range(n):
            if m == j:
                continue
            xm = F.from_i64(m)
            lj = poly_mul(lj, [F.neg(xm), 1])
            denom = F.mul(denom, F.sub(xj, xm))
        scale = F.div(yj, denom)
        for k, l in enumerate(lj):
            coeffs[k] = (coeffs[k] + scale * l) % M
    return coeffs


def poly_evaluate(coeffs, x):  # polynomials.rs:9-14
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % M
    return acc


def to_polynomial(nonzero, s):  # sumcheck.rs:269-276
    a0 = F.div(F.sub(s, sum(nonzero) % M), 2)
    return [a0] + list(nonzero)


# ---- evaluation.rs -----------------------------------------------------------

def mask_evaluate(index, n_vars, points):  # evaluation.rs:56-73
    acc = 1
    for i in range(n_vars):
        p = points[n_vars - 1 - i]
        acc = acc * (p if (index >> i) & 1 else (1 - p)) % M
    return acc


def delta_evaluate(data, points):  # evaluation.rs:80-90
    acc = 1
    for a, b in zip(data, points):
        acc = acc * ((a * b + (1 - a) * (1 - b)) % M) % M
    return acc


def trace_evaluate(matrix, width, points):  # evaluation.rs:31-48
    n = len(points)
    res = [0] * width
    for row in range(len(matrix) // width):
        c = mask_evaluate(row, n, points)
        for j in range(width):
            res[j] = (res[j] + c * matrix[row * width + j]) % M
    return res


# ---- system.rs ---------------------------------------------------------------

class ChallengeSet:  # system.rs:131-146
    def __init__(self, transcript, num_randoms, log_num_constraints, log_num_rows):
        # vec![x; n] evaluates x once; next_challenge() absorbs nothing
        self.row = [transcript.next_challenge()] * log_num_rows
        self.trace = [transcript.next_challenge()] * num_randoms
        self.constraint = [transcript.next_challenge()] * log_num_constraints


class System:
    """constraints: callables f(var, rand) -> int in [0, M); degree: the
    declared composition degree; matrix: row-major list (None: verifier)."""

    def __init__(self, transcript, constraints, degree, columns, randoms, log_num_rows,
                 matrix=None):  # system.rs:74-104
        self.constraints = list(constraints)
        self.degree = degree
        self.columns = columns
        self.matrix = matrix
        n = len(self.constraints)
        log_nc = max(n - 1, 0).bit_length()  # next_power_of_two().trailing_zeros()
        self.challenges = ChallengeSet(transcript, randoms, log_nc, log_num_rows)
        self.constraint_mask = [mask_evaluate(i, log_nc, self.challenges.constraint)
                                for i in range(n)]

    def evaluate_composition(self, outputs):  # evaluation.rs:5-11,21-29
        assert len(outputs) == self.columns
        rnd = self.challenges.trace
        acc = 0
        for f, mk in zip(self.constraints, self.constraint_mask):
            acc = (acc + mk * f(outputs, rnd)) % M
        return acc

    def evaluate_delta(self, inputs):  # evaluation.rs:13-18
        assert len(inputs) == len(self.challenges.row)
        return delta_evaluate(self.challenges.row, inputs)

    def build_tables(self):  # sumcheck.rs:22-38
        height = len(self.matrix) // self.columns
        n_vars = height.bit_length() - 1
        row = self.challenges.row
        delta = [mask_evaluate(i, n_vars, row) for i in range(height)]
        return SumcheckTables(list(self.matrix), self.columns, height, delta)

    def compute_sumcheck_polynomials(self, transcript, tables, total):  # sumcheck.rs:40-53
        return tables.compute_sumcheck_polynomials(self.evaluate_composition, self.degree,
                                                   transcript, total)

    def _replay(self, transcript, pols, total):  # sumcheck.rs:61-79 / :98-116
        rs = []
        for c in pols[0]:
            transcript.absorb(F.to_bytes(c))
        pol = to_polynomial(pols[0], total)
        for sp in pols[1:]:
            r = transcript.next_challenge()
            for c in sp:
                transcript.absorb(F.to_bytes(c))
            pol = to_polynomial(sp, poly_evaluate(pol, r))
            rs.append(r)
        r = transcript.next_challenge()
        rs.append(r)
        return rs, poly_evaluate(pol, r)

    def verify_sumcheck_debug(self, transcript, pols, total):  # sumcheck.rs:55-89
        rs, val = self._replay(transcript, pols, total)
        output = trace_evaluate(self.matrix, self.columns, rs)
        assert F.mul(self.evaluate_delta(rs), self.evaluate_composition(output)) == val, \
            "Does not match polynomial evaluation"

    def verify_with_evaluations(self, transcript, pols, total, output):  # sumcheck.rs:91-124
        rs, val = self._replay(transcript, pols, total)
        assert F.mul(self.evaluate_delta(rs), self.evaluate_composition(output)) == val, \
            "Does not match polynomial evaluation"


# ---- sumcheck.rs -------------------------------------------------------------

class SumcheckTables:  # sumcheck.rs:10-15
    def __init__(self, matrix, width, height, delta):
        self.matrix = matrix
        self.width = width
        self.height = height
        self.delta = delta

    def compute_sumcheck_polynomials(self, composition, degree, transcript, total):  # :147-172
        pols, randoms = [], []
        previous = total
        total_degree = degree + 1
        n_rounds = self.height.bit_length() - 1
        for _ in range(n_rounds):
            pol, r, previous = self.compute_sumcheck_polynomial(composition, total_degree,
                                                                previous, transcript)
            pols.append(pol)
            randoms.append(r)
        return pols, randoms

    def compute_sumcheck_polynomial(self, composition, total_degree, previous, transcript):
        """:174-202 -> (nonzero coefficients, r, new previous_sum)."""
        evals = [0] * (total_degree + 1)
        for i in range(1, total_degree + 1):
            evals[i] = self.partial_sum(composition, F.from_i64(i))
        evals[0] = F.sub(previous, evals[1])
        pol = interpolate(evals)
        nonzero = pol[1:]
        for c in nonzero:
            transcript.absorb(F.to_bytes(c))
        r = transcript.next_challenge()
        previous = poly_evaluate(pol, r)
        self.fold(r)
        return nonzero, r, previous

    def partial_sum(self, composition, r):  # :204-232
        off = self.height >> 1
        w, mat, dl = self.width, self.matrix, self.delta
        tot = 0
        if r == 1:
            for i in range(off):
                d = r * dl[i + off] % M
                m = [r * mat[(i + off) * w + j] % M for j in range(w)]
                tot += composition(m) * d
            return tot % M
        s = (1 - r) % M
        for i in range(off):
            d = (s * dl[i] + r * dl[i + off]) % M
            m = [(s * mat[i * w + j] + r * mat[(i + off) * w + j]) % M for j in range(w)]
            tot += composition(m) * d
        return tot % M

    def fold(self, r):  # :234-247
        self.height >>= 1
        off = self.height
        w, mat, dl = self.width, self.matrix, self.delta
        s = (1 - r) % M
        for i in range(off):
            dl[i] = (s * dl[i] + r * dl[i + off]) % M
            for j in range(w):
                mat[i * w + j] = (s * mat[i * w + j] + r * mat[(i + off) * w + j]) % M
        # (the reference keeps the stale second half; nothing reads it again)
        del dl[off:]
        del mat[off * w:]
