"""CPU checks of the shortened butterfly chains (tools/gen_bfly.py): the
instruction counts, and that operands built to lose each ripple the asm leaves
out (E: carry out of limb 2 of the fold; FA / FD: carry / borrow out of limb 1
of the wrap correction) raise that flag in the emulated asm and come out exact
after the cold path.

Counts against the targets 55 / 16 / 42 / 61 / 8 VALU per butterfly of kinds
m / t / p / f / c: 55, 16, 41, 60 and 8.  The products alone (p, f) cannot drop
limb 3 of their sum as the butterfly does; they fold the top word into the
sum's low limbs instead and flag the borrow that this leaves out (G)."""
import pytest

import bfly_rare_cases as R

G = R.gen()
TOP = (1 << 128) - 1
TARGET = {"m": 55, "t": 16, "p": 42, "f": 61, "c": 8}


@pytest.mark.parametrize("kinds", G.VARIANTS, ids="".join)
def test_valu_count(kinds):
    lines = G.render(kinds, "v")[0]
    valu = sum(1 for ln in lines if ln.startswith("v_"))
    print(kinds, "VALU", valu, "s_nop", sum(int(ln.split()[1]) + 1 for ln in lines if ln.startswith("s_nop")))
    assert valu <= sum(TARGET[k] for k in kinds)


def _run(kinds, slot, u, v, w):
    """Emulate `kinds` with (u, v, w) in butterfly `slot` and harmless operands
    in the other; return this butterfly's flags (E, FA, FD) and fixed (a, d)."""
    lines, _, _, _, _, nv, opn = G.render(kinds, "v")
    G.check_hazards(lines)
    uv = [3] * len(kinds)
    vv = [5] * len(kinds)
    wv = [1] * len(kinds)
    uv[slot], vv[slot], wv[slot] = u, v, (1 if w is None else w)
    regs = G.run_regs(kinds, lines, opn, uv, vv, wv)
    flag = lambda f: regs["%%%d" % opn["%s%d" % (f, slot)]] if "%s%d" % (f, slot) in opn else 0
    res = G.run_case(kinds, lines, opn, nv, uv, vv, wv)
    for b, (a, d) in enumerate(res):  # every butterfly of the statement is exact
        ww = wv[b] if kinds[b] == "m" else 1
        assert 0 <= a < (1 << 128) and 0 <= d < (1 << 128)
        assert a % G.M == (uv[b] + ww * vv[b]) % G.M and d % G.M == (uv[b] - ww * vv[b]) % G.M, (kinds, b)
    return (flag("E"), flag("FA"), flag("FD")), res[slot]


# (variant, slot) pairs that hold a trivial butterfly / one with a twiddle
TRIVIAL = [(("t",), 0), (("t", "t"), 0), (("t", "t"), 1), (("m", "t"), 1)]
TWIDDLED = [(("m",), 0), (("m", "m"), 0), (("m", "m"), 1), (("m", "t"), 0)]


@pytest.mark.parametrize("kinds,slot", TRIVIAL + TWIDDLED)
def test_fa_and_fd_directed(kinds, slot):
    """u = M-1, v = 2^64 + C loses the carry of a; u = 0, v = 2^64 - 5 the
    borrow of d (w = 1 stands for the trivial butterfly in the twiddled
    kinds: its product is v itself)."""
    w = None if kinds[slot] == "t" else 1
    for a, b in ((0, 0), (7, 3), (G.C - 1, 0), (G.C - 1, G.C - 1)):
        u, v = R.fa_pair(a, b)
        assert G.model(u, v, w)[2:] == (0, 1, 0)  # the model finds the flag ...
        assert _run(kinds, slot, u, v, w)[0] == (0, 1, 0)  # ... and the asm raises it
    for a, b in ((0, 0), (7, 3), (G.C - 6, 0), (0, G.C - 6)):
        u, v = R.fd_pair(a, b)
        assert G.model(u, v, w)[2:] == (0, 0, 1)
        assert _run(kinds, slot, u, v, w)[0] == (0, 0, 1)


@pytest.mark.parametrize("kinds,slot", TRIVIAL + TWIDDLED)
def test_fa_with_fd_and_cold_add_wrapping(kinds, slot):
    w = None if kinds[slot] == "t" else 1
    # both flags: u + v = 2^128 + 2^64 - 1, u - v = -(2^64 - 5)
    u, v = (1 << 127) + 2, (1 << 127) + (1 << 64) - 3
    assert _run(kinds, slot, u, v, w)[0] == (0, 1, 1)
    # u = v = 2^128 - 1: a = 2^128 - 2^64 + ... and its + 2^64 wraps 2^128 again
    a, _, _, fa, _ = G.model(TOP, TOP, w)
    assert fa == 1 and a + (1 << 64) >= (1 << 128)
    flags, (ga, gd) = _run(kinds, slot, TOP, TOP, w)
    assert flags == (0, 1, 0) and ga == G.relaxed_add(a, 1 << 64) and ga < (1 << 64) + 2 * G.C
    # the same for d: u - v = 5 - 2^128, so d < 2^64 and d - 2^64 borrows out of 2^128
    _, d, _, _, fd = G.model(0, TOP - 4, w)
    assert fd == 1 and d < (1 << 64)
    flags, (ga, gd) = _run(kinds, slot, 0, TOP - 4, w)
    assert flags == (0, 0, 1) and gd == G.relaxed_sub(d, 1 << 64) and gd > (1 << 128) - (1 << 64) - 2 * G.C


@pytest.mark.parametrize("kinds,slot", TWIDDLED)
@pytest.mark.parametrize("inverse", [False, True])
def test_e_directed(kinds, slot, inverse):
    """v from a search over the model for w = omega_4 loses the fold's carry;
    with u chosen after the product, E meets FA, and E meets FD."""
    w = R.omega4(inverse)
    for v in R.e_operands(w):
        assert G.model(0, v, w)[2] == 1
        assert _run(kinds, slot, 12345, v, w)[0][0] == 1
        # s as the asm holds it (u = 0: a = s), without its lost 2^96
        s = G.model(0, v, w)[0]
        # E + FA: u + s = 2^128 + 2^64 - 1
        u = (1 << 128) + (1 << 64) - 1 - s
        if 0 <= u < (1 << 128):
            assert _run(kinds, slot, u, v, w)[0][:2] == (1, 1)
        # E + FD: u - s = -(2^64 - 5)
        u = s - (1 << 64) + 5
        if 0 <= u < (1 << 128):
            flags, _ = _run(kinds, slot, u, v, w)
            assert flags[0] == 1 and flags[2] == 1
    # the cold path's + 2^96 itself wraps: a = u + s with limb 3 all ones
    v = R.e_operands(w)[0]
    s = G.model(0, v, w)[0]
    u = ((1 << 128) - (1 << 96) + (s & ((1 << 96) - 1)) - s) % (1 << 128)
    a, _, fe, _, _ = G.model(u, v, w)
    assert fe == 1 and a + (1 << 96) >= (1 << 128)
    flags, (ga, _) = _run(kinds, slot, u, v, w)
    assert flags == (1, 0, 0) and ga == G.relaxed_add(a, 1 << 96) and ga < (1 << 96) + 2 * G.C


PRODUCTS = [(("p",), 0), (("p", "p"), 0), (("p", "p"), 1), (("f",), 0), (("f", "f"), 0), (("f", "f"), 1)]


@pytest.mark.parametrize("kinds,slot", PRODUCTS)
def test_products_g_and_k_directed(kinds, slot):
    """Operands that lose the fold's borrow out of limb 1 (G), in either
    slot and either operand order, and operands that carry out of 2^128 (K):
    the emulated asm raises the flag and the fixed product is exact."""
    lines, _, _, _, _, nv, opn = G.render(kinds, "v")
    G.check_hazards(lines)

    def run(v, w):
        vv, wv = [5] * len(kinds), [7] * len(kinds)
        vv[slot], wv[slot] = v, w
        regs = G.run_regs(kinds, lines, opn, [0] * len(kinds), vv, wv)
        res = G.run_case(kinds, lines, opn, nv, [0] * len(kinds), vv, wv)
        for b, (_, d) in enumerate(res):
            assert 0 <= d < (1 << 128) and d % G.M == vv[b] * wv[b] % G.M, (kinds, b)
        return regs["%%%d" % opn["K%d" % slot]], regs["%%%d" % opn["G%d" % slot]]

    if kinds[slot] == "p":
        assert run(*R.G_PAIR_P) == (0, 1)
        assert run(TOP, 2)[0] == 1  # 2 (2^128 - 1): the sum carries out of 2^128
    else:
        for v, w in R.G_PAIRS_F:
            assert R.full_product_g(v, w) == 1 and R.full_product_g(w, v) == 1
            assert run(v, w)[1] == 1 and run(w, v)[1] == 1
        assert run((1 << 127) - 2, TOP)[0] == 1  # test_bfly_asm's carry case


@pytest.mark.parametrize("kinds", G.VARIANTS, ids="".join)
@pytest.mark.parametrize("seed", [11, 12])
def test_selftest_long(kinds, seed):
    """20 000 random and edge operand sets per variant (the edge list holds
    2^64-1, 2^64-C, 2^64-C-1, 2^96-1 and 2^96)."""
    lines, _, _, _, _, nv, opn = G.render(kinds, "v")
    assert G.selftest(kinds, lines, opn, nv, trials=20000, seed=seed) == 20000 * len(kinds)
