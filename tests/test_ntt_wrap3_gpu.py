"""GPU: the three-instruction wrap correction of the butterflies (bfly_asm.hpp)
at its boundaries, bit-exact against the C oracle.

The correction adds C = 0x2D00 2^32 - 1 to a sum that wrapped out of 2^128 as
"- 1 into limb 0, + 0x2D00 into limb 1" (and the mirror image for a difference
that borrowed).  The - 1 borrows into limb 1 exactly when limb 0 of the
wrapped sum is 0, and the lost carry FA is then set iff limb 1 >= 0xFFFFD301;
the + 1 carries exactly when limb 0 of the wrapped difference is 0xFFFFFFFF,
and FD is then set iff limb 1 < 0x2CFF.  Four boundary cases, one on each side
of both thresholds:

  sum_keep   wrapped sum (0, 0xFFFFD300, ..): the borrow reaches limb 1, FA clear
  sum_flag   wrapped sum (0, 0xFFFFD301, ..): the borrow reaches limb 1, FA set
  diff_keep  wrapped difference (0xFFFFFFFF, 0x2CFF, ..): the carry reaches limb 1, FD clear
  diff_flag  wrapped difference (0xFFFFFFFF, 0x2CFE, ..): the carry reaches limb 1, FD set

All four occur with canonical operands (u = M - 1 - r and v = X + C + 1 + r
give u + v = 2^128 + X; u = r and v = 2^128 - Y + r give u - v = Y - 2^128), so
none is left out.  The pairs sit where a transform's first butterflies (w = 1)
meet them -- the pair layout of test_ntt_rare_paths_gpu.py, whose FA / FD / E
operands keep every second slot of theirs -- and before the GPU is touched the
first stage is replayed on integers: each case has to come up at least 64
times in one period, with the flag the derivation gives.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_ntt_addressing_gpu as AD  # noqa: E402
import test_ntt_rare_paths_gpu as RP  # noqa: E402
from oracle import field as F  # noqa: E402

from multilinear_amd import device as D  # noqa: E402
from multilinear_amd import ntt as MN  # noqa: E402

G = RP.G
TOP = 1 << 128
M32 = (1 << 32) - 1
# case -> (slot of the pair in a group of 8, low limbs of the wrapped result, flag)
CASES = {
    "sum_keep": (3, (0, 0xFFFFD300), 0),
    "sum_flag": (4, (0, 0xFFFFD301), 1),
    "diff_keep": (5, (M32, 0x2CFF), 0),
    "diff_flag": (7, (M32, 0x2CFE), 1),
}
PER_PERIOD = RP.PERIOD // 8


def _pairs(case, seed):
    """PER_PERIOD canonical pairs (u, v) of one case: random upper limbs of
    the wrapped result, a random split between the operands."""
    import random

    r = random.Random(seed)
    _, (l0, l1), _ = CASES[case]
    out = []
    for _ in range(PER_PERIOD):
        res = l0 | (l1 << 32) | (r.randrange(1 << 32) << 64) | (r.randrange(1, 1 << 31) << 96)
        k = r.randrange(1 << 20)
        if case.startswith("sum"):
            u, v = G.M - 1 - k, res + G.C + 1 + k
            assert u + v == TOP + res
        else:
            u, v = k, TOP - res + k
            assert u - v == res - TOP
        assert 0 <= u < G.M and 0 <= v < G.M
        out.append((u, v))
    return out


def wrap3_vector(n, seed, layout):
    """rare_vector of that file with the four cases in slots 3, 4, 5, 7 of
    every group of 8 pairs (its FA and FD pairs keep slots 0 and 1, its E
    operands theirs)."""
    x = RP.rare_vector(n, seed, layout)
    h = n // 2
    q = h // 2 if layout == "ntt" else h
    for i, (case, (slot, _, _)) in enumerate(sorted(CASES.items())):
        pairs = _pairs(case, seed * 8 + i)
        rows = len(range(slot, q, 8))
        x[slot:q:8] = np.resize(D.ints_to_limbs([u for u, _ in pairs]), (rows, 4))
        x[h + slot:h + q:8] = np.resize(D.ints_to_limbs([v for _, v in pairs]), (rows, 4))
    return x


def replay_boundary_counts(x):
    """How often each case comes up in the first period's w = 1 butterflies
    (x[j], x[j + n/2]) -- stage 0 of a transform, stage 1 of an encoding -- by
    the generator's integer model, with the flag checked."""
    h = x.shape[0] // 2
    cnt = dict.fromkeys(CASES, 0)
    us, vs = D.limbs_to_ints(x[0:RP.PERIOD]), D.limbs_to_ints(x[h:h + RP.PERIOD])
    for u, v in zip(us, vs):
        _, _, _, fa, fd = G.model(u, v, None)
        for case, (_, low, flag) in CASES.items():
            if case.startswith("sum"):
                hit = u + v >= TOP and ((u + v) & M32, ((u + v) >> 32) & M32) == low
                got = fa
            else:
                hit = u < v and ((u - v) & M32, ((u - v) >> 32) & M32) == low
                got = fd
            if hit:
                assert got == flag, (case, u, v)
                cnt[case] += 1
    return cnt


def _check_counts(x, layout):
    counts = replay_boundary_counts(x)
    flags = RP.replay_flag_counts(x, layout)
    print("%s layout, n = %d: boundary cases %s, E / FA / FD %s in one period" % (layout, x.shape[0], counts, flags))
    assert min(counts.values()) >= 64, counts
    assert min(flags) >= 64, flags


@functools.lru_cache(maxsize=None)
def _case(log_n, layout):
    """Vector, replay (asserted) and oracle transforms of one size, computed once."""
    C = AD._c_oracle()
    n = 1 << log_n
    g = F.pow_2_generator(log_n if layout == "ntt" else log_n + 1)
    x = wrap3_vector(n, 5000 + log_n, layout)
    _check_counts(x, layout)
    if layout == "rs":
        return x, g, C.reed_solomon_par(x, log_n, g), None
    return x, g, C.ntt_par(x, log_n, g), C.ntt_par(x, log_n, g, inverse=True) if log_n <= 16 else None


def test_default_plan_narrow_and_wide():
    """2^11, the smallest size that uses the pass kernels: forward and inverse
    through the narrow and the wide kernels."""
    x, g, fwd, inv = _case(11, "ntt")
    AD._both("", "ntt", x, x.shape[0], fwd, 11, D.fe_bytes(g))
    AD._both("", "intt", x, x.shape[0], inv, 11, D.fe_bytes(g))


def test_forced_plan_8_8():
    """2^16 as two radix-2^8 passes: all three register phases, twiddles from
    scalar registers (phase 1) and from the LDS copy (phases 2 and 3)."""
    x, g, fwd, inv = _case(16, "ntt")
    AD._both("8,8", "ntt", x, x.shape[0], fwd, 16, D.fe_bytes(g))
    AD._both("8,8", "intt", x, x.shape[0], inv, 16, D.fe_bytes(g))


def test_reed_solomon_2_11_to_2_12():
    """The zero-padded first pass copies u to v in stage 0, so the pairs meet
    in stage 1."""
    x, g, code, _ = _case(11, "rs")
    AD._both("", "rs", x, 2 * x.shape[0], code, 11, D.fe_bytes(g))


def test_progression_pass0():
    """2^23, the smallest size whose pass 0 takes its twiddles as a
    progression (TW 5); the forward transform."""
    x, g, fwd, _ = _case(23, "ntt")
    RP._same(D.from_device(MN.Polynomial(D.to_device(x)).ntt(g).evals), fwd)
