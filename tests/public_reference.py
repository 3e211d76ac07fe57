"""Plain-Python model of the system proof with public columns
(mlh_system_prove_public / mlh_system_verify_public), for
tests/test_public_*.py.  No libmlhip arithmetic and no closed form: it composes
the parts tests/shifted_reference.py composes,

  tests/cs_reference.py                   System on the extension E, SumcheckTables
                                          again for the shift reduction
  tests/phased_reference.py               the sumcheck with sum columns
  tests/system_reference.py               _open: the batched-PCS openings
  oracle.transcript                       Transcript

in the order of include/mlhip.h: the SHA-256 of the spec's wire bytes absorbed
first, steps 1-7 of the shifted proof on all W columns, the commitments and
the openings over the columns [0, P) and [P, W - F) only.  The public columns
are built by plain indexing from a description -- a list of ("const", c),
("first",), ("last",), ("row",), ("periodic", values), ("sparse", {row: value})
-- and the values a verifier derives are the explicit sum over the rows against
cs_reference.mask_evaluate (public_at).

Constraints are callables f(var, rand) over the W + K wide row of E.
"""
import ctypes
import functools
import hashlib
import random
import struct

import cs_reference as R
import phased_reference as PR
import shifted_reference as SR
import system_reference as S
from oracle import field as F
from oracle import transcript as OT

M = F.M
KINDS = {"const": 0, "first": 1, "last": 2, "row": 3, "periodic": 4, "sparse": 5}


# ---- the spec ---------------------------------------------------------------------

def wire(descs):
    """The wire format of include/mlhip.h, encoded here on its own."""
    b = struct.pack("<2I", len(descs), 0)
    for d in descs:
        kind = KINDS[d[0]]
        if d[0] == "const":
            b += struct.pack("<2I", kind, 0) + F.to_bytes(d[1])
        elif d[0] == "periodic":
            b += struct.pack("<2I", kind, len(d[1]).bit_length() - 1)
            b += b"".join(F.to_bytes(v) for v in d[1])
        elif d[0] == "sparse":
            b += struct.pack("<2I", kind, len(d[1]))
            b += b"".join(struct.pack("<Q", r) + F.to_bytes(v) for r, v in sorted(d[1].items()))
        else:
            b += struct.pack("<2I", kind, 0)
    return b


def column(d, H):
    """One public column over H rows, by plain indexing."""
    if d[0] == "const":
        return [d[1]] * H
    if d[0] == "first":
        return [1 if i == 0 else 0 for i in range(H)]
    if d[0] == "last":
        return [1 if i == H - 1 else 0 for i in range(H)]
    if d[0] == "row":
        return list(range(H))
    if d[0] == "periodic":
        return [d[1][i % len(d[1])] for i in range(H)]
    return [d[1].get(i, 0) for i in range(H)]


def strip(descs, H):
    """The H x F strip, row-major."""
    cols = [column(d, H) for d in descs]
    return [c[i] for i in range(H) for c in cols]


def public_at(descs, L, point):
    """The columns' multilinear extensions at `point`: the sum over the rows."""
    H = 1 << L
    eq = [R.mask_evaluate(i, L, point) for i in range(H)]
    return [sum(e * v for e, v in zip(eq, column(d, H))) % M for d in descs]


def with_strip(committed, C, descs, H):
    """The H x (C + F) matrix of the committed columns and the spec's strip."""
    st, Fn, out = strip(descs, H), len(descs), []
    for i in range(H):
        out += committed[i * C:(i + 1) * C] + st[i * Fn:(i + 1) * Fn]
    return out


# ---- the proof ----------------------------------------------------------------------

def prove(seed, fns, degree, width, randoms, log_height, matrix, pre, sum_columns, shifts, descs,
          total=None, column_sum=None):
    """-> dict: the proof's parts in host form and the transcript digests.
    matrix: all W columns, the public strip as the prover holds it (a wrong
    strip gives a proof the verifier rejects)."""
    P, W, K, L, Fn = pre, width, len(shifts), log_height, len(descs)
    H, Wx, C = 1 << L, width + len(shifts), width - len(descs)
    E = SR.extend(matrix, W, shifts, H)
    columns = S.columns_of(matrix, W)
    columns1, columns2 = columns[:P], columns[P:C]
    root1 = S.batch_root(columns1, L)
    root2 = S.batch_root(columns2, L) if P < C else None
    spec_wire = wire(descs)
    spec_digest = hashlib.sha256(spec_wire).digest()
    ot = OT.Transcript()
    ot.absorb(seed)
    entry = ot.random()
    prefix = seed
    if Fn:
        ot.absorb(spec_digest)                                             # 0
        prefix += spec_digest
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
    beta = 0
    prefix += root1 + (root2 or b"")
    if sum_columns:                                                        # 5
        ot.absorb(F.to_bytes(column_sum))
        prefix += F.to_bytes(column_sum)
        beta = ot.next_challenge()
    claim = (total + beta * column_sum) % M
    pols, rs, output = PR.sumcheck(sysm, ot, sum_columns, beta, claim)     # 6
    after_sumcheck = ot.random()
    coeff_bytes = b"".join(F.to_bytes(c) for p in pols for c in p)
    prefix += coeff_bytes
    pols2, rs2, output2, shift_bytes, lam, after_shift = [], [], [], b"", None, None
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
        after_shift = ot.random()
    openings = []
    pcs, pcs_shift = [], []
    for at, vals, dst in ((rs, output, pcs), (rs2, output2, pcs_shift)):   # 8
        if dst is pcs_shift and not K:
            break
        p1, prefix = S._open(ot, prefix, at, vals[:P], columns1, L, openings)
        dst.append(p1)
        assert p1["batch_commitment"] == root1
        if P < C:
            p2, prefix = S._open(ot, prefix, at, vals[P:C], columns2, L, openings)
            dst.append(p2)
            assert p2["batch_commitment"] == root2
    digest = ot.random()
    return dict(seed=seed, entry=entry, root1=root1, root2=root2, sysm=sysm, matrix=matrix,
                extension=E, total=total, column_sum=column_sum, beta=beta, claim=claim,
                trace_randoms=trace_randoms, pols=pols, rs=rs, output=output,
                after_sumcheck=after_sumcheck, coeff_bytes=coeff_bytes, lam=lam, pols2=pols2,
                rs2=rs2, output2=output2, shift_bytes=shift_bytes, after_shift=after_shift,
                pcs=pcs, pcs_shift=pcs_shift, digest=digest, log_height=L, width=W, degree=degree,
                pre=P, sum_columns=tuple(sum_columns), mask=PR.column_mask(sum_columns),
                randoms=randoms, shifts=list(shifts), fns=fns, descs=list(descs), wire=spec_wire,
                spec_digest=spec_digest, n_public=Fn, committed=C)


# ---- the systems ---------------------------------------------------------------

def pfib_exprs():
    """(a, b | first, last, io): Fibonacci with a statement -- next(a) = b and
    next(b) = a + b on every row but the last, a = io on the first row, b = io
    on the last."""
    from multilinear_amd.constraint_system import nxt, var

    return [(1 - var(3)) * (nxt(0) - var(1)), (1 - var(3)) * (nxt(1) - var(0) - var(1)),
            var(2) * (var(0) - var(4)), var(3) * (var(1) - var(4))]


PFIB_FNS = [lambda v, r: (1 - v[3]) * (v[5] - v[1]) % M,
            lambda v, r: (1 - v[3]) * (v[6] - v[0] - v[1]) % M,
            lambda v, r: v[2] * (v[0] - v[4]) % M,
            lambda v, r: v[3] * (v[1] - v[4]) % M]


def fib_columns(log_height, a=1, b=1):
    """The committed columns a, b (H x 2) and b on the last row."""
    out, last = [], None
    for _ in range(1 << log_height):
        out += [a, b]
        last = b
        a, b = b, (a + b) % M
    return out, last


def pfib_descs(log_height, result, start=1):
    H = 1 << log_height
    return [("first",), ("last",), ("sparse", {0: start, H - 1: result})]


def pmixed_exprs():
    """(x0, x1 | x2, x3 | c, row, per): W = 7, one random, one shift whose
    source is the public row-index column; unsatisfied on a random trace."""
    from multilinear_amd.constraint_system import nxt, rand, var

    return [nxt(5) - var(5) - rand(0) * var(0) * var(1) + var(4),
            var(3) * var(1) - nxt(5) * var(0) + var(6) * var(2)]


PMIXED_FNS = [lambda v, r: (v[7] - v[5] - r[0] * v[0] * v[1] + v[4]) % M,
              lambda v, r: (v[3] * v[1] - v[7] * v[0] + v[6] * v[2]) % M]


def pwide_exprs():
    """W = 20 (4 committed, 16 public), K = 12 in the order nxt(19), nxt(18),
    ...: the 32-column limit."""
    from multilinear_amd.constraint_system import nxt, var

    e = nxt(19) * var(0)
    for k in range(1, 12):
        e = e + nxt(19 - k) * var(k)
    return [e]


PWIDE_FNS = [lambda v, r: sum(v[20 + k] * v[k] for k in range(12)) % M]


def _random_list(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(M) for _ in range(n)]


def pwide_descs(log_height):
    H = 1 << log_height
    v = _random_list(21, 64 + H)
    return [("const", v[0]), ("first",), ("last",), ("row",), ("periodic", v[1:2]),
            ("periodic", v[2:10]), ("periodic", v[64:64 + H]), ("sparse", {H - 1: v[10]}),
            ("sparse", {0: v[11], 1: v[12], H // 2: v[13], H - 1: v[14]}), ("const", 0),
            ("row",), ("last",), ("first",), ("periodic", v[15:17]), ("sparse", {0: v[17]}),
            ("const", M - 1)]


# name -> (exprs, fns, degree, W, randoms, L, matrix, P, sum columns, shifts, descs, total)
def _system(name):
    if name.startswith("pfib") and name[4:].isdigit():
        L = int(name[4:])
        ab, result = fib_columns(L)
        descs = pfib_descs(L, result)
        return (pfib_exprs, PFIB_FNS, 2, 5, 0, L, with_strip(ab, 2, descs, 1 << L), 2, (), [0, 1],
                descs, 0)
    if name == "pmixed5":
        descs = [("const", 12345678901234567890123), ("row",), ("periodic", _random_list(31, 4))]
        m = with_strip(_random_list(32, 4 << 5), 4, descs, 1 << 5)
        return (pmixed_exprs, PMIXED_FNS, 3, 7, 1, 5, m, 2, (3,), [5], descs, None)
    if name == "pwide9":
        descs = pwide_descs(9)
        m = with_strip(_random_list(33, 4 << 9), 4, descs, 1 << 9)
        return (pwide_exprs, PWIDE_FNS, 2, 20, 0, 9, m, 2, (1,), list(range(19, 7, -1)), descs, None)
    if name == "pfib4_wrong_start":  # a trace started from a != io[0]
        ab, result = fib_columns(4, a=2, b=1)
        descs = pfib_descs(4, result)
        return (pfib_exprs, PFIB_FNS, 2, 5, 0, 4, with_strip(ab, 2, descs, 16), 2, (), [0, 1],
                descs, 0)
    raise KeyError(name)


GPU_NAMES = ["pfib1", "pfib4", "pfib9", "pmixed5", "pwide9", "pfib13"]
CPU_NAMES = ["pfib1", "pfib4", "pmixed5"]
SEED = b"public"


def exprs(name):
    return _system(name)[0]()


def descs(name):
    return _system(name)[10]


def program(name):
    """-> (wire, shift list) by multilinear_amd's compile step."""
    from multilinear_amd.constraint_system import compile_shifted

    ex, _, degree, W, randoms = _system(name)[:5]
    return compile_shifted(ex(), W, randoms, degree)


def builder(ds):
    """The description as a multilinear_amd PublicColumns."""
    from multilinear_amd.constraint_system import PublicColumns

    pc = PublicColumns()
    for d in ds:
        {"const": pc.const, "first": pc.first, "last": pc.last, "row": pc.row_index,
         "periodic": pc.periodic, "sparse": pc.sparse}[d[0]](*d[1:])
    return pc


@functools.lru_cache(maxsize=None)
def model(name):
    _, fns, degree, W, randoms, L, matrix, P, sc, shifts, ds, total = _system(name)
    return prove(SEED, fns, degree, W, randoms, L, matrix, P, sc, shifts, ds, total=total)


def pack(mo):
    """A model proof as mlh_shifted_proof: a multilinear_amd ShiftedSystemProof
    (the buffer holder) filled with the model's bytes."""
    from multilinear_amd.constraint_system import ShiftedSystemProof

    p = ShiftedSystemProof(mo["log_height"], mo["width"], mo["degree"], mo["pre"], mo["mask"],
                           mo["shifts"], mo["n_public"])
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
