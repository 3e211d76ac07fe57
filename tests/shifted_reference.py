"""Plain-Python model of the shifted system proof (mlh_system_prove_shifted /
mlh_system_verify_shifted), for tests/test_shifted_proof_*.py.  No libmlhip
arithmetic and no closed form: it composes

  the extension E by plain indexing       E[i][W + k] = T[(i + 1) mod H][c_k]
  tests/cs_reference.py                   System on E; SumcheckTables again for
                                          the shift reduction, its delta list
                                          the eq list of rs rotated by one row
  tests/phased_reference.py               the sumcheck with sum columns
  oracle.transcript                       Transcript
  oracle.batched.BatchedPCSProof.prove    the four openings (above 2^9 rows the
                                          C oracle through the absorbed-bytes
                                          prefix, as phased_reference)

in the order of include/mlhip.h: steps 1-5 of the phased proof, the sumcheck
on E, absorb output, lambda, the shift sumcheck of

  sum_j succ[j] sum_k lambda^k T[j][c_k] = sum_k lambda^k output[W + k],

the openings of columns [0, P) and [P, W) at (rs, output[0:W]) and again at
(rs', output2).  succ(rs, rs') is the explicit sum over the rows.

Constraints are callables f(var, rand) over the W + K wide row of E.
"""
import ctypes
import functools
import random

import cs_reference as R
import phased_reference as PR
import system_reference as S
from oracle import field as F
from oracle import transcript as OT

M = F.M


def extend(matrix, W, shifts, H):
    out = []
    for i in range(H):
        out += matrix[i * W:(i + 1) * W]
        nx = (i + 1) % H
        out += [matrix[nx * W + c] for c in shifts]
    return out


def succ_brute(x, y):
    """sum_i eq(x, i) eq(y, (i + 1) mod 2^n), row by row."""
    n = len(x)
    H = 1 << n
    return sum(R.mask_evaluate(i, n, x) * R.mask_evaluate((i + 1) % H, n, y) for i in range(H)) % M


def prove(seed, fns, degree, width, randoms, log_height, matrix, pre, sum_columns, shifts,
          total=None, column_sum=None):
    """-> dict: the proof's parts in host form and the transcript digests."""
    P, W, K, L = pre, width, len(shifts), log_height
    H, Wx = 1 << L, width + len(shifts)
    E = extend(matrix, W, shifts, H)
    columns = S.columns_of(matrix, W)
    columns1, columns2 = columns[:P], columns[P:]
    root1 = S.batch_root(columns1, L)
    root2 = S.batch_root(columns2, L) if P < W else None
    ot = OT.Transcript()
    ot.absorb(seed)
    entry = ot.random()
    ot.absorb(root1)                                                       # 1
    trace_randoms = [ot.next_challenge()] * randoms                        # 2
    if root2 is not None:
        ot.absorb(root2)                                                   # 3
    sysm = R.System(ot, fns, degree, Wx, randoms, L, E)                    # 4
    sysm.challenges.trace = trace_randoms
    delta = [R.mask_evaluate(i, L, sysm.challenges.row) for i in range(H)]
    if total is None:
        total = sum(d * sysm.evaluate_composition(E[i * Wx:(i + 1) * Wx])
                    for i, d in enumerate(delta)) % M
    if column_sum is None:
        column_sum = sum(matrix[i * W + j] for i in range(H) for j in sum_columns) % M
    beta, prefix = 0, seed + root1 + (root2 or b"")
    if sum_columns:                                                        # 5
        ot.absorb(F.to_bytes(column_sum))
        prefix += F.to_bytes(column_sum)
        beta = ot.next_challenge()
    claim = (total + beta * column_sum) % M
    pols, rs, output = PR.sumcheck(sysm, ot, sum_columns, beta, claim)     # 6
    after_sumcheck = ot.random()
    coeff_bytes = b"".join(F.to_bytes(c) for p in pols for c in p)
    prefix += coeff_bytes
    pols2, rs2, output2, shift_bytes, lam, succ_val, after_shift = [], [], [], b"", None, None, None
    if K:                                                                  # 7
        out_bytes = b"".join(F.to_bytes(v) for v in output)
        ot.absorb(out_bytes)
        prefix += out_bytes
        lam = ot.next_challenge()
        lams = [pow(lam, k, M) for k in range(K)]
        claim2 = sum(lams[k] * output[W + k] for k in range(K)) % M
        eq_rs = [R.mask_evaluate(i, L, rs) for i in range(H)]
        succ = [eq_rs[(j - 1) % H] for j in range(H)]
        tables2 = R.SumcheckTables(list(matrix), W, H, succ)

        def comp(row):
            return sum(lams[k] * row[c] for k, c in enumerate(shifts)) % M

        pols2, rs2 = tables2.compute_sumcheck_polynomials(comp, 1, ot, claim2)
        output2 = tables2.matrix[:W]
        shift_bytes = b"".join(F.to_bytes(c) for p in pols2 for c in p)
        prefix += shift_bytes
        succ_val = succ_brute(rs, rs2)
        assert tables2.delta[0] == succ_val
        after_shift = ot.random()
    openings = []
    pcs, pcs_shift = [], []
    for at, vals, dst in ((rs, output, pcs), (rs2, output2, pcs_shift)):   # 8
        if dst is pcs_shift and not K:
            break
        p1, prefix = S._open(ot, prefix, at, vals[:P], columns1, L, openings)
        dst.append(p1)
        assert p1["batch_commitment"] == root1
        if P < W:
            p2, prefix = S._open(ot, prefix, at, vals[P:W], columns2, L, openings)
            dst.append(p2)
            assert p2["batch_commitment"] == root2
    digest = ot.random()
    return dict(seed=seed, entry=entry, root1=root1, root2=root2, sysm=sysm, matrix=matrix,
                extension=E, total=total, column_sum=column_sum, beta=beta, claim=claim,
                trace_randoms=trace_randoms, pols=pols, rs=rs, output=output,
                after_sumcheck=after_sumcheck, coeff_bytes=coeff_bytes, lam=lam, pols2=pols2,
                rs2=rs2, output2=output2, shift_bytes=shift_bytes, succ=succ_val,
                after_shift=after_shift, pcs=pcs, pcs_shift=pcs_shift, digest=digest,
                log_height=L, width=W, degree=degree, pre=P, sum_columns=tuple(sum_columns),
                mask=PR.column_mask(sum_columns), randoms=randoms, shifts=list(shifts), fns=fns)


# ---- the systems ---------------------------------------------------------------

def fib_exprs():
    """(a, b, last): next(a) = b and next(b) = a + b on every row but the last."""
    from multilinear_amd.constraint_system import nxt, var

    return [(1 - var(2)) * (nxt(0) - var(1)), (1 - var(2)) * (nxt(1) - var(0) - var(1))]


FIB_FNS = [lambda v, r: (1 - v[2]) * (v[3] - v[1]) % M,
           lambda v, r: (1 - v[2]) * (v[4] - v[0] - v[1]) % M]


def fib_matrix(log_height, restart_at=None, ungated_wrap=False):
    """The Fibonacci trace; restart_at = i: the sequence starts afresh (from 5,
    3) at row i, so that exactly the step i - 1 -> i breaks; ungated_wrap: last
    is 0 on the last row too, so that exactly the wrap H - 1 -> 0 breaks."""
    H = 1 << log_height
    a, b, out = 1, 1, []
    for i in range(H):
        if restart_at is not None and i == restart_at:
            a, b = 5, 3
        out += [a, b, 1 if (i == H - 1 and not ungated_wrap) else 0]
        a, b = b, (a + b) % M
    return out


def mixed_exprs():
    """W = 4, one random, one shift: unsatisfied on a random trace."""
    from multilinear_amd.constraint_system import nxt, rand, var

    return [nxt(2) - var(2) - rand(0) * var(0) * var(1), var(3) * var(1) - nxt(2) * var(0)]


MIXED_FNS = [lambda v, r: (v[4] - v[2] - r[0] * v[0] * v[1]) % M,
             lambda v, r: (v[3] * v[1] - v[4] * v[0]) % M]


def wide_exprs():
    """W = 16, K = 16, in the order nxt(15), nxt(14), ...: the 32-column limit."""
    from multilinear_amd.constraint_system import nxt, var

    e = nxt(15) * var(0)
    for k in range(1, 16):
        e = e + nxt(15 - k) * var(k)
    return [e]


WIDE_FNS = [lambda v, r: sum(v[16 + k] * v[k] for k in range(16)) % M]


def _random_matrix(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(M) for _ in range(n)]


# name -> (exprs, fns, degree, W, randoms, L, matrix, P, sum columns, shifts, total)
def _system(name):
    if name.startswith("fib") and name[3:].isdigit():
        L = int(name[3:])
        return (fib_exprs, FIB_FNS, 2, 3, 0, L, fib_matrix(L), 3, (), [0, 1], 0)
    if name == "mixed5":
        return (mixed_exprs, MIXED_FNS, 3, 4, 1, 5, _random_matrix(11, 4 << 5), 2, (3,), [2], None)
    if name == "wide9":
        return (wide_exprs, WIDE_FNS, 2, 16, 0, 9, _random_matrix(12, 16 << 9), 5, (1,),
                list(range(15, -1, -1)), None)
    if name == "fib_broken_mid":
        return (fib_exprs, FIB_FNS, 2, 3, 0, 4, fib_matrix(4, restart_at=7), 3, (), [0, 1], 0)
    if name == "fib_broken_wrap":
        return (fib_exprs, FIB_FNS, 2, 3, 0, 4, fib_matrix(4, ungated_wrap=True), 3, (), [0, 1], 0)
    raise KeyError(name)


GPU_NAMES = ["fib1", "fib4", "fib9", "mixed5", "wide9", "fib13"]
CPU_NAMES = ["fib1", "fib4", "mixed5"]
SEED = b"shifted"


def exprs(name):
    return _system(name)[0]()


def program(name):
    """-> (wire, shift list) by multilinear_amd's compile step."""
    from multilinear_amd.constraint_system import compile_shifted

    ex, _, degree, W, randoms = _system(name)[:5]
    return compile_shifted(ex(), W, randoms, degree)


@functools.lru_cache(maxsize=None)
def model(name):
    _, fns, degree, W, randoms, L, matrix, P, sc, shifts, total = _system(name)
    return prove(SEED, fns, degree, W, randoms, L, matrix, P, sc, shifts, total=total)


def pack(mo):
    """A model proof as mlh_shifted_proof: a multilinear_amd ShiftedSystemProof
    (the buffer holder) filled with the model's bytes."""
    from multilinear_amd.constraint_system import ShiftedSystemProof

    p = ShiftedSystemProof(mo["log_height"], mo["width"], mo["degree"], mo["pre"], mo["mask"],
                           mo["shifts"])
    ctypes.memmove(p._polys, mo["coeff_bytes"], len(mo["coeff_bytes"]))
    out = b"".join(F.to_bytes(v) for v in mo["output"])
    ctypes.memmove(p._output, out, len(out))
    if mo["shifts"]:
        ctypes.memmove(p._shift_polys, mo["shift_bytes"], len(mo["shift_bytes"]))
        out2 = b"".join(F.to_bytes(v) for v in mo["output2"])
        ctypes.memmove(p._output2, out2, len(out2))
    for i, pcs in enumerate(mo["pcs"]):
        S._fill_pcs(p.pcs[i], p.c.pcs[i], pcs)
    for i, pcs in enumerate(mo["pcs_shift"]):
        S._fill_pcs(p.pcs_shift[i], p.c.pcs_shift[i], pcs)
    p._sync()
    return p
