"""CPU: the butterflies' three-instruction wrap correction and the generated
cold-path statements (tools/gen_bfly.py), on the generator's emulator.

The correction of a wrap out of 2^128 (+ C on the sum side, - C on the
difference side, C = 0x2D00 2^32 - 1) is two carry instructions and one select
per side; the lost carry out of limb 1 is C1 AND NOT borrow-out (B1 AND NOT
carry-out), taken on the SALU.  It is the same 64-bit sum as before, so every
statement must return model()'s (a, d, E, FA, FD) bit for bit.

The boundaries follow from the arithmetic.  With (l0, l1) the low limbs of the
wrapped sum, the sum side computes l1 + 0x2D00 - [l0 = 0]: FA is set iff
l1 >= 0xFFFFD300 + [l0 = 0].  With (l0, l1) those of the wrapped difference,
the difference side computes l1 - 0x2D00 + [l0 = 0xFFFFFFFF]: FD is set iff
l1 + [l0 = 0xFFFFFFFF] < 0x2D00.
"""
import importlib.util
import itertools
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_bfly", os.path.join(ROOT, "tools", "gen_bfly.py"))
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)

TOP = 1 << 128
M32 = (1 << 32) - 1
BFLY_VARIANTS = [k for k in G.VARIANTS if any(x in ("m", "t") for x in k)]
# VALU per statement before this change (the committed header's stats lines)
VALU_BEFORE = {("p", "p"): 82, ("p",): 41, ("f", "f"): 120, ("f",): 60, ("c", "c", "c", "c"): 32, ("c",): 8}
VALU_BOUND = {"m": 53, "t": 14}


def _sources(kinds):
    return ("s", "v") if any(k in ("m", "p") for k in kinds) else ("v",)


def _valu(lines):
    return sum(1 for l in lines if l.startswith("v_"))


@pytest.mark.parametrize("kinds", G.VARIANTS)
def test_instruction_counts(kinds):
    for bsrc in _sources(kinds):
        n = _valu(G.render(kinds, bsrc)[0])
        if kinds in VALU_BEFORE:
            assert n <= VALU_BEFORE[kinds], (kinds, n)
        else:
            assert n <= sum(VALU_BOUND[k] for k in kinds), (kinds, n)


@pytest.mark.parametrize("kinds", G.VARIANTS + [("x",), ("y",)])
def test_hazards(kinds):
    for bsrc in _sources(kinds):
        G.check_hazards(G.render(kinds, bsrc)[0])


def test_hazard_checker_knows_the_salu_rule():
    """A VALU read of a VALU-written mask one instruction later is refused; a
    SALU read of it, and a VALU read of what the SALU wrote, are not."""
    w = "v_add_co_u32_e64 v0, %1, v1, v2"
    with pytest.raises(AssertionError):
        G.check_hazards([w, "v_cndmask_b32_e64 v3, 0, 1, %1"])
    G.check_hazards([w, "s_andn2_b64 %2, %1, %3", "v_cndmask_b32_e64 v3, 0, 1, %2"])
    G.check_hazards([w, "s_nop 1", "v_cndmask_b32_e64 v3, 0, 1, %1"])


def _raw(kinds, lines, opn, uv, vv, wv):
    """The statement's outputs before the cold path: [(a, d, E, FA, FD)]."""
    regs = G.run_regs(kinds, lines, opn, uv, vv, wv)
    out = []
    for b, k in enumerate(kinds):
        hi = "x" if k == "t" else "u"
        a = G.value([regs["%%%d" % opn["%s%d_%d" % ("u" if i < 2 else hi, b, i)]] for i in range(4)])
        d = G.value([regs["%%%d" % opn["v%d_%d" % (b, i)]] for i in range(4)])
        fe = regs["%%%d" % opn["E%d" % b]] if k == "m" else 0
        out.append((a, d, fe, regs["%%%d" % opn["FA%d" % b]], regs["%%%d" % opn["FD%d" % b]]))
    return out


def _roots():
    g = pow(3, (G.M - 1) >> 9, G.M)
    return [w for w in (pow(g, e, G.M) for e in range(512)) if w != G.M - 1]


@pytest.mark.parametrize("kinds", BFLY_VARIANTS)
def test_statement_equals_model_on_selftest_mix(kinds):
    """20 000 seeded trials of selftest's operand mix (30 % edge values, stage
    twiddles of order <= 2^9)."""
    C, M = G.C, G.M
    edge = [0, 1, M - 1, M, TOP - 1, C, C - 1, TOP - C, TOP - C - 1, M - C, 1 << 127, (1 << 96) - 1, M32,
            (TOP - 1) ^ M32, (1 << 64) - 1, (1 << 64) - C, (1 << 64) - C - 1, 1 << 96]
    roots = _roots()
    lines, _, _, _, _, _, opn = G.render(kinds, "v")
    rng = random.Random(20000)
    pick = lambda: rng.choice(edge) if rng.random() < 0.3 else rng.randrange(TOP)
    for _ in range(20000):
        uv = [pick() for _ in kinds]
        vv = [pick() for _ in kinds]
        wv = [rng.choice(roots) for _ in kinds]
        got = _raw(kinds, lines, opn, uv, vv, wv)
        for b, k in enumerate(kinds):
            assert got[b] == G.model(uv[b], vv[b], wv[b] if k == "m" else None), (kinds, b, uv[b], vv[b], wv[b])


def boundary_operands():
    """(u, s, side, wraps, l0, l1): u + s (side 'a') or u - s (side 'd') whose
    low limbs are (l0, l1), wrapping / borrowing or not (the twin)."""
    out = []
    rng = random.Random(3)
    his = [0, 1, (1 << 63) - 1]  # limbs 2, 3 of the result (below 2^127: room for both operands)
    for l0, l1, hi in itertools.product([0, 1, M32], [0, 0xFFFFD2FF, 0xFFFFD300, 0xFFFFD301, M32], his):
        X = l0 | (l1 << 32) | (hi << 64)
        for wraps in (True, False):
            # u + s = 2^128 + X, or = X with the same low limbs
            total = X + (TOP if wraps else 0)
            s = rng.randrange(max(0, total - TOP + 1), min(TOP, total + 1))
            out.append((total - s, s, "a", wraps, l0, l1))
    his[0] = 2  # (a difference of exactly -2^128 does not exist)
    for l0, l1, hi in itertools.product([0, 1, M32], [0, 0x2CFE, 0x2CFF, 0x2D00, M32], his):
        Y = l0 | (l1 << 32) | (hi << 64)
        for wraps in (True, False):
            # u - s = Y - 2^128, or = Y
            diff = Y - (TOP if wraps else 0)
            s = rng.randrange(max(0, -diff), min(TOP, TOP - diff))
            out.append((s + diff, s, "d", wraps, l0, l1))
    return out


BOUNDARY = boundary_operands()


def test_boundary_operands_are_what_they_say():
    assert len(BOUNDARY) == 2 * 2 * 3 * 5 * 3
    for u, s, side, wraps, l0, l1 in BOUNDARY:
        assert 0 <= u < TOP and 0 <= s < TOP
        r = u + s if side == "a" else u - s
        assert (r >= TOP if side == "a" else r < 0) == wraps
        assert r & M32 == l0 and (r >> 32) & M32 == l1


@pytest.mark.parametrize("kinds", BFLY_VARIANTS)
def test_statement_equals_model_on_boundaries(kinds):
    """Every boundary operand in every butterfly slot of the statement (kind m
    with w = 1, whose product is v itself), the other slots random."""
    lines, _, _, _, _, _, opn = G.render(kinds, "v")
    rng = random.Random(5)
    roots = _roots()
    for slot in range(len(kinds)):
        for u, s, side, wraps, l0, l1 in BOUNDARY:
            uv = [rng.randrange(TOP) for _ in kinds]
            vv = [rng.randrange(TOP) for _ in kinds]
            wv = [rng.choice(roots) for _ in kinds]
            uv[slot], vv[slot], wv[slot] = u, s, 1
            got = _raw(kinds, lines, opn, uv, vv, wv)
            for b, k in enumerate(kinds):
                assert got[b] == G.model(uv[b], vv[b], wv[b] if k == "m" else None), (kinds, b, uv[b], vv[b])
            a, d, fe, fa, fd = got[slot]
            assert fe == 0
            if side == "a":
                assert fa == (1 if wraps and l1 >= 0xFFFFD300 + (l0 == 0) else 0), (u, s, fa)
                if not wraps:  # limbs 0 and 1 left alone
                    assert a & ((1 << 64) - 1) == l0 | (l1 << 32)
            else:
                assert fd == (1 if wraps and l1 + (l0 == M32) < 0x2D00 else 0), (u, s, fd)
                if not wraps:
                    assert d & ((1 << 64) - 1) == l0 | (l1 << 32)


def test_fix_statement_equals_fix():
    """The butterflies' cold path as a statement: fix() on every flag
    combination, active and inactive lanes, over operands at every distance
    the add-backs turn on and random ones."""
    lines, _, _, _, _, _, opn = G.render(("x",), "v")
    rng = random.Random(11)
    ops = G.fix_operands() + [rng.randrange(TOP) for _ in range(64)]
    for a, d in itertools.product(ops, ops[::3]):
        for fe, fa, fd in itertools.product((0, 1), repeat=3):
            assert G.run_fix(lines, opn, a, d, fe, fa, fd) == G.fix(a, d, fe, fa, fd) + (1,), (a, d, fe, fa, fd)
    for a, d in zip(ops, reversed(ops)):
        for fe, fa, fd in itertools.product((0, 1), repeat=3):
            assert G.run_fix(lines, opn, a, d, fe, fa, fd, active=0) == (a, d, 0)


def test_fix_statement_rewraps():
    """The add-back wraps once: a = 2^128 - 1 with any flag, d = 0 with any
    flag; the + C / - C of that wrap is applied.  A second wrap (the second
    round of relaxed_add / relaxed_sub, which the statement carries as fix()
    does) needs a wrapped value within C of 2^128 (of 0), and the largest
    add-back, 2^96 + 2^64, leaves it below 2^97 (above 2^128 - 2^97): it
    cannot occur, which the extremes below show; both rounds are still checked
    against fix() on every operand of fix_operands()."""
    lines, _, _, _, _, _, opn = G.render(("x",), "v")
    C = G.C
    for fe, fa, fd in itertools.product((0, 1), repeat=3):
        y = (fa << 64) + (fe << 96)
        z = (fd << 64) + (fe << 96)
        a, d, ex = G.run_fix(lines, opn, TOP - 1, 0, fe, fa, fd)
        assert ex == 1
        assert a == (TOP - 1 + y - TOP + C if y else TOP - 1)
        assert d == (TOP - z - C if z else 0)
        assert (a, d) == G.fix(TOP - 1, 0, fe, fa, fd)
        if y:  # once wrapped, far from wrapping again
            assert a + C < TOP
        if z:
            assert d - C > 0


def test_prod_fix_statement_equals_prod_fix():
    lines, _, _, _, _, _, opn = G.render(("y",), "v")
    rng = random.Random(13)
    ops = G.fix_operands() + [G.M - 1, G.M, G.M + 1] + [rng.randrange(TOP) for _ in range(256)]
    for v in ops:
        for fk, fg in itertools.product((0, 1), repeat=2):
            assert G.run_prod_fix(lines, opn, v, fk, fg) == (G.prod_fix(v, fk, fg), 1), (v, fk, fg)
            assert G.run_prod_fix(lines, opn, v, fk, fg, active=0) == (v, 0)
    # the + C wraps (v >= M) and the - 2^64 then borrows or not; v < 2^64 borrows at once
    for v in (TOP - 1, G.M, (1 << 64) - 1, 0):
        got, _ = G.run_prod_fix(lines, opn, v, 1, 1)
        assert got % G.M == (v + G.C - (1 << 64)) % G.M and 0 <= got < TOP
