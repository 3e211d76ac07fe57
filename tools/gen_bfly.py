"""Generator for the hand-scheduled gfx950 radix-2 butterflies (multilinear_amd/csrc/bfly_asm.hpp).

Why: the NTT passes are VALU-issue bound.  hipcc cannot use the
carry-out of v_mad_u64_u32, so the field product was written as one small asm
statement per multiply-accumulate; every statement boundary then costs a pad
and every carry a 2-state SGPR hazard (gfx950: a VALU write of an SGPR/VCC must
be 2 wait states ahead of a VALU read of it), ~1.5 `s_nop` per mad.  This tool
emits whole butterflies (one or two per statement, interleaved) with the
hazards covered by independent work, in the RELAXED representation:

  values are any representative in [0, 2^128) (2M > 2^128, so every residue
  has one or two), canonicalised only where they leave the NTT.

Butterfly (DIT): (u, v) -> (u + w*v, u - w*v), w given as its four limb-shifted
multiples B_k = w * 2^(32k) mod M ("expanded" stage twiddles, fe_mul_pre):
  * product: 16 v_mad_u64_u32 column-scanned, carries counted by v_addc;
    T = top bits (< 2^34) folded once: s = r + x, x = T*C < 2^80,
    C = 2^128 - M = 0x2D00*2^32 - 1.  x has three limbs, so only limbs 0..2
    are added and limb 3 of s is r3 itself; the carry out of limb 2
    (x2 < 2^16: probability ~2^-17) is flagged (E: true s = s + 2^96).
  * a = u + s: a carry out of 2^128 (C1) is worth + C, a 46-bit constant,
    which is added to limbs 0 and 1 only; limbs 2 and 3 of the first sum are
    final.  + C = - 1 + 0x2D00 2^32 takes three instructions: limb 0 minus
    C1 as a borrow-in, a select of - 0x2D00 (0xFFFFD300, operand kneg) or 0,
    limb 1 minus that and the borrow.  The carry out of limb 1 (low64 + C >=
    2^64: ~2^-18.5 for the values a transform carries) happened exactly when
    C1 is set and the last borrow-out is clear: one s_andn2_b64 gives the
    flag (FA: true a = a + 2^64).
  * d = u - s: borrow (B1) -> - C on limbs 0 and 1 by the mirror image (two
    v_addc and the same select); the borrow out of limb 1 is B1 and not the
    last carry-out (FD: true d = d - 2^64).
  53 VALU per butterfly with a twiddle (31 product, 5 fold, 3 s, 8 u +- s,
  6 corrections), 14 without, no s_nop in the paired variants.
The flags are SGPR lane masks; the C++ wrapper ORs them on the SALU and
branches to a cold path that adds the lost ripples back in relaxed
arithmetic: a += FA*2^64 + E*2^96, d -= FD*2^64 + E*2^96, where a wrap out of
2^128 is worth +-C (and that C may wrap once more).  The cold path is a
generated statement too (kinds 'x' and 'y', fix_prog / prod_fix_prog: the
limbs are in/out operands and the work runs under an EXEC mask built from
the flags), so that the block the branch enters leaves every value in the
register it has and the compiler needs no copies where it rejoins the hot
path; fix() / prod_fix() below and bfly_fix / prod_fix in the header say in
plain arithmetic what it computes.  At 2^-17 per lane a few hundred waves
per 2^24-point pass take the branch.  The fixes do not depend on how often
the flags fire, only the time does.

Products alone ('p': v <- w v by expanded multiples, any twiddle, 41 VALU;
'f': v <- w v by a plain table entry, 60 VALU) keep the carry into limb 3,
and their flag K is the carry out of 2^128 (true v = s + C).  In 'p' r3 sits
in a physical register pair and needs an instruction to reach its operand
whatever that instruction does; in 'f' the folded word reaches 2^93, so the
carry out of limb 2 is not rare (about 1 lane in 100).  They save two
instructions in the fold instead (fold_add_prog): the - T of
T*C = (T*0x2D00 << 32) - T is taken from the sum's limbs 0 and 1 directly,
and the borrow out of limb 1 (r1 < t_hi + 1: ~2^-30 in 'p', ~2^-20 in 'f')
is flagged (G: true v = v - 2^64).

A trivial butterfly reads u and v in both u + v and u - v, so the first of
the two cannot overwrite either: limbs 2 and 3 of a leave the statement in
write-only operands, which the wrapper assigns to u (a register rename).

Precondition of the product (checked by tests/test_bfly_asm.py over every
stage twiddle the NTT can use): the first mad of columns 1..3 adds
v0*B0[j] to a carry word < 2^35, which cannot overflow 64 bits when
B0[j] = w's limb j <= 2^32 - 8.  Every root of unity of order <= 2^9 except -1
satisfies it, and -1 is never a stage twiddle (j < len/2).

The same instruction list drives a one-lane emulator and a hazard checker
(`emulate`, `check_hazards`), so the asm is validated on the CPU before it
ever runs.  Run:  python tools/gen_bfly.py   (rewrites bfly_asm.hpp)
"""
import os
import random

M = (1 << 128) - 45 * (1 << 40) + 1
C = (1 << 128) - M
MASK32 = (1 << 32) - 1
KC1 = C >> 32  # 0x2CFF
K2D00 = 0x2D00
KNEG = (-K2D00) & MASK32  # 0xFFFFD300: limb 1 of the wrap correction, negated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "multilinear_amd", "csrc", "bfly_asm.hpp")

# VGPR temporaries live in physical registers (pairs must be even-aligned and
# their halves addressable, which an inline-asm operand cannot give).
VBASE = 0

# ---------------------------------------------------------------- program ---


class Ins:
    """One instruction.  dst/src name virtual registers (str) or immediates (int).
    A pair is ('pair', lo, hi).  sdst/cin name SGPR-pair virtual registers."""

    def __init__(self, op, dst, src, sdst=None, cin=None, tag=0, after=(), sin=()):
        self.op, self.dst, self.src, self.sdst, self.cin, self.tag = op, dst, src, sdst, cin, tag
        # SGPR-pair sources of a SALU instruction ('sandn2': sdst = sin[0] AND NOT
        # sin[1]; 'sor': OR; 'saveexec': sdst = EXEC, EXEC &= sin[0]; 'restexec': EXEC = sin[0])
        self.sin = tuple(sin)
        # names whose every read must precede this instruction (it reuses
        # their register: the second hi partner of a pair's lo, see allocate)
        self.after = tuple(after)

    def vreads(self):
        out = []
        for s in self.src:
            if isinstance(s, tuple):
                out += [s[1], s[2]]
            elif isinstance(s, str):
                out.append(s)
        return out

    def vwrites(self):
        if isinstance(self.dst, tuple):
            return [self.dst[1], self.dst[2]]
        return [self.dst] if self.dst else []

    def sreads(self):
        return ([self.cin] if self.cin else []) + list(self.sin)

    def is_salu(self):
        return self.op in ("sandn2", "sor", "saveexec", "restexec")

    def swrites(self):
        return [self.sdst] if self.sdst and self.sdst != "junk" else []


def fold_add_prog(E, p, R, t_lo, t_hi, S, b):
    """S = R + T*C for the products alone (kinds 'p', 'f'), seven instructions:
    T*C = (T*0x2D00 << 32) - T, and the - T goes straight into R's limbs 0 and
    1 instead of into a word of its own.  The borrow out of limb 1
    (R1 < t_hi + 1: ~2^-30 in 'p', ~2^-20 in 'f') is left out and flagged
    (G: true S = S - 2^64); K is the carry out of 2^128 (true S = S + C)."""
    Y = ("pair", p + "Y.lo", p + "Y.hi")
    E("mad", Y, [t_lo, "k2d00", 0], sdst="junk")
    E("mad24", p + "Yh2", [t_hi, "k2d00", Y[2]])
    E("sub", S[0], [R[0], t_lo], sdst=p + "bb5")
    E("subb", p + "m1", [R[1], t_hi], sdst="G%d" % b, cin=p + "bb5")
    E("add", S[1], [p + "m1", Y[1]], sdst=p + "e1")
    E("addc", S[2], [R[2], p + "Yh2"], sdst=p + "e2", cin=p + "e1")
    E("addc", S[3], [R[3], 0], sdst="K%d" % b, cin=p + "e2")


def product_prog(E, p, V, B, safe):
    """t = sum_k V_k * B_k (relaxed), appended through E.  safe: count the carry
    of every column's first mad too (any twiddle); otherwise columns 1..3 rely
    on the stage-twiddle precondition (module docstring).  Returns the four
    limb names of r (the low four columns) and, with safe, the top word's
    (t_lo, t_hi) unfolded; otherwise the folded top word is left in x0..x2.
    The caller adds the two."""
    r = []
    acc = 0
    for j in range(4):
        cys = []
        for k in range(4):
            dst = ("pair", p + "P%d_%d.lo" % (j, k), p + "P%d_%d.hi" % (j, k))
            if k == 0 and (j == 0 or not safe):
                E("mad", dst, [V[k], B[k][j], acc], sdst="junk")
            else:
                cy = p + "cy%d%d" % (j, k)
                cys.append(cy)
                E("mad", dst, [V[k], B[k][j], acc], sdst=cy)
            acc = dst
        r.append(acc[1])
        # carry count -> hi half of the next column's addend pair
        nlo, nhi = p + "Q%d.lo" % (j + 1), p + "Q%d.hi" % (j + 1)
        c = 0
        for n, cy in enumerate(cys):
            d = nhi if n == len(cys) - 1 else p + "c%d_%d" % (j, n)
            E("addc", d, [c, 0], sdst="junk", cin=cy)
            c = d
        if j < 3:
            E("mov", nlo, [acc[2]])
            acc = ("pair", nlo, nhi)
        else:
            t_lo, t_hi = acc[2], nhi
    if safe:  # the product alone: the caller folds and adds in one go
        return r, (t_lo, t_hi)
    # fold T*2^128 = T*C = T*0x2D00*2^32 - T
    Y = ("pair", p + "Y.lo", p + "Y.hi")
    E("mad", Y, [t_lo, "k2d00", 0], sdst="junk")
    E("mad24", p + "Yh2", [t_hi, "k2d00", Y[2]])
    E("sub", p + "x0", [0, t_lo], sdst=p + "bb0")
    E("subb", p + "x1", [Y[1], t_hi], sdst=p + "bb1", cin=p + "bb0")
    E("subb", p + "x2", [p + "Yh2", 0], sdst="junk", cin=p + "bb1")
    return r, None


def fmul_prog(E, p, V, W):
    """Full product v * w of two plain 128-bit values (w: a table entry, any
    value < 2^128), relaxed result written to the tied output d.  Product
    scan over 7 columns (16 mads; the first mad of columns 0, 1 and the single
    mad of column 6 cannot overflow, every other carry is counted), then
    H*2^128 = H*C = H*0x2D00*2^32 - H: Z = L + (H*0x2D00 << 32) by 4 mads,
    Z - H (limbs x0..x3) with its top T = (tl, th) < 2^47, which the caller
    folds once more (fold_add_prog).  That add keeps all four limbs: T*C
    reaches 2^93 here, so the carry out of limb 2 is set in about one lane in
    a hundred (measured with the emulator) and nearly every second wave would
    take a cold path for it."""
    acc = 0
    r = []
    col_hi = {}
    for j in range(7):
        terms = [(i, j - i) for i in range(4) if 0 <= j - i <= 3]
        cys = []
        for n, (i, jj) in enumerate(terms):
            dst = ("pair", p + "P%d_%d.lo" % (j, n), p + "P%d_%d.hi" % (j, n))
            if (n == 0 and j <= 1) or j == 6:
                E("mad", dst, [V[i], W[jj], acc], sdst="junk")
            else:
                cy = p + "cy%d%d" % (j, n)
                cys.append(cy)
                E("mad", dst, [V[i], W[jj], acc], sdst=cy)
            acc = dst
        r.append(acc[1])
        col_hi[j] = acc[2]
        if j == 6:
            r.append(acc[2])
            break
        nlo, nhi = p + "Q%d.lo" % (j + 1), p + "Q%d.hi" % (j + 1)
        if cys:
            c = 0
            for n, cy in enumerate(cys):
                d = nhi if n == len(cys) - 1 else p + "c%d_%d" % (j, n)
                E("addc", d, [c, 0], sdst="junk", cin=cy)
                c = d
        else:
            E("mov", nhi, [0])
        E("mov", nlo, [acc[2]])
        acc = ("pair", nlo, nhi)
    # Z = L + (H * 0x2D00) << 32.  Z_j = r_j + r_{j+3}*0x2D00 (j = 1..3) by a
    # mad onto the pair {r_j, 0}: r_j's own register pair, whose hi half
    # (the column's carry word, already moved on) is re-zeroed; Z_4 = r_7*0x2D00.
    Z = {}
    for j in (1, 2, 3):
        zr = p + "Zr%d" % j
        E("mov", zr, [0], after=[col_hi[j]])
        Z[j] = ("pair", p + "Z%d.lo" % j, p + "Z%d.hi" % j)
        E("mad", Z[j], [r[j + 3], "k2d00", ("pair", r[j], zr)], sdst="junk")
    Z[4] = ("pair", p + "Z4.lo", p + "Z4.hi")
    E("mad", Z[4], [r[7], "k2d00", 0], sdst="junk")
    # carry words (< 2^15) into the next limb
    E("add", p + "a2", [Z[2][1], Z[1][2]], sdst=p + "e3")
    E("addc", p + "a3", [Z[3][1], Z[2][2]], sdst=p + "e4", cin=p + "e3")
    E("addc", p + "a4", [Z[4][1], Z[3][2]], sdst=p + "e5", cin=p + "e4")
    E("addc", p + "a5", [Z[4][2], 0], sdst="junk", cin=p + "e5")
    # X = Z - H (>= 0): x0..x3, top T = (tl, th) < 2^47
    E("sub", p + "x0", [r[0], r[4]], sdst=p + "bb0")
    E("subb", p + "x1", [Z[1][1], r[5]], sdst=p + "bb1", cin=p + "bb0")
    E("subb", p + "x2", [p + "a2", r[6]], sdst=p + "bb2", cin=p + "bb1")
    E("subb", p + "x3", [p + "a3", r[7]], sdst=p + "bb3", cin=p + "bb2")
    E("subb", p + "tl", [p + "a4", 0], sdst=p + "bb4", cin=p + "bb3")
    E("subb", p + "th", [p + "a5", 0], sdst="junk", cin=p + "bb4")
    return [p + "x0", p + "x1", p + "x2", p + "x3"], (p + "tl", p + "th")


def canon_prog(E, p, b):
    """Relaxed -> canonical: x >= M iff x + C carries out of 2^128."""
    V = ["v%d_%d" % (b, i) for i in range(4)]
    T = [p + "T%d" % i for i in range(4)]
    E("add", T[0], [V[0], -1], sdst=p + "e0")
    E("addc", T[1], [V[1], "kc1"], sdst=p + "e1", cin=p + "e0")
    E("addc", T[2], [V[2], 0], sdst=p + "e2", cin=p + "e1")
    E("addc", T[3], [V[3], 0], sdst=p + "e3", cin=p + "e2")
    for i in range(4):
        E("cnd", "d%d_%d" % (b, i), [V[i], T[i]], cin=p + "e3")


def wrap_rounds(E, p, tag, cur, wrap, out, sub):
    """Two rounds of "a wrap out of 2^128 is worth C": cur (four limb names)
    + C (- C with sub) where the SGPR mask wrap is set, then once more on
    the carry (borrow) of that; the second cannot wrap again.  The last
    round writes the names in out.  Returns nothing: out holds the result."""
    first, nxt = ("sub", "subb") if sub else ("add", "addc")
    for r in (1, 2):
        new = out if r == 2 else [p + "%s%d_%d" % (tag, r, i) for i in range(4)]
        cy = [p + "f%s%d_%d" % (tag, r, i) for i in range(4)]
        m0, m1 = p + "m%s%d_0" % (tag, r), p + "m%s%d_1" % (tag, r)
        E("cnd", m0, [0, -1], cin=wrap)
        E("cnd", m1, [0, p + "kc"], cin=wrap)
        E(first, new[0], [cur[0], m0], sdst=cy[0])
        E(nxt, new[1], [cur[1], m1], sdst=cy[1], cin=cy[0])
        E(nxt, new[2], [cur[2], 0], sdst=cy[2], cin=cy[1])
        E(nxt, new[3], [cur[3], 0], sdst=cy[3] if r == 1 else "junk", cin=cy[2])
        cur, wrap = new, cy[3]


def fix_prog(E, p, b):
    """Kind 'x', the butterflies' cold path as a statement: (a, d) <-
    fix(a, d, fe, fa, fd) with the three flags as SGPR lane masks (inputs sE,
    sFA, sFD).  The butterfly's limbs are in/out operands, so the block that
    holds this statement defines them in the registers they already have.
    Runs under EXEC = EXEC AND (fe OR fa OR fd): the other lanes keep their
    values.  a += fa 2^64 + fe 2^96, d -= fd 2^64 + fe 2^96, then the two
    possible re-wraps of relaxed_add / relaxed_sub.  Emitted in program order
    (its cost is paid by a few hundred waves per pass)."""
    U = ["u%d_%d" % (b, i) for i in range(4)]
    V = ["v%d_%d" % (b, i) for i in range(4)]
    fe, fa, fd = "sE%d" % b, "sFA%d" % b, "sFD%d" % b
    E("sor", None, [], sdst=p + "em0", sin=[fe, fa])
    E("sor", None, [], sdst=p + "em1", sin=[p + "em0", fd])
    E("saveexec", None, [], sdst=p + "esave", sin=[p + "em1"])
    E("cnd", p + "ya", [0, 1], cin=fa)
    E("cnd", p + "yd", [0, 1], cin=fd)
    E("cnd", p + "ye", [0, 1], cin=fe)
    E("mov", p + "kc", [KC1])
    for tag, X, y2, sub in (("a", U, p + "ya", False), ("d", V, p + "yd", True)):
        first, nxt = ("sub", "subb") if sub else ("add", "addc")
        cur = [X[0], X[1], p + tag + "0_2", p + tag + "0_3"]
        E(first, cur[2], [X[2], y2], sdst=p + "f%s0_2" % tag)
        E(nxt, cur[3], [X[3], p + "ye"], sdst=p + "f%s0_3" % tag, cin=p + "f%s0_2" % tag)
        wrap_rounds(E, p, tag, cur, p + "f%s0_3" % tag, ["%s%d_%d" % (tag, b, i) for i in range(4)], sub)
    E("restexec", None, [], sin=[p + "esave"])


def prod_fix_prog(E, p, b):
    """Kind 'y', the products' cold path as a statement (as fix_prog):
    v <- v + fk C - fg 2^64 in relaxed arithmetic, flags sK and sG."""
    V = ["v%d_%d" % (b, i) for i in range(4)]
    fk, fg = "sK%d" % b, "sG%d" % b
    E("sor", None, [], sdst=p + "em0", sin=[fk, fg])
    E("saveexec", None, [], sdst=p + "esave", sin=[p + "em0"])
    E("cnd", p + "yg", [0, 1], cin=fg)
    E("mov", p + "kc", [KC1])
    K = [p + "k%d" % i for i in range(4)]
    wrap_rounds(E, p, "k", V, fk, K, False)
    cur = [K[0], K[1], p + "s0_2", p + "s0_3"]
    E("sub", cur[2], [K[2], p + "yg"], sdst=p + "fs0_2")
    E("subb", cur[3], [K[3], 0], sdst=p + "fs0_3", cin=p + "fs0_2")
    wrap_rounds(E, p, "s", cur, p + "fs0_3", ["d%d_%d" % (b, i) for i in range(4)], True)
    E("restexec", None, [], sin=[p + "esave"])


def bfly_prog(b, kind):
    """Instruction list of butterfly b.  kind 'm': with a stage twiddle, 't':
    trivial (w = 1), 'p': product only v <- w v (safe first mads; any twiddle).
    Operand names: u{b}_{i} (in, tied to a), v{b}_{i} (in, tied to d),
    B{b}_{k}{j} (twiddle limbs), kneg (VGPR 0xFFFFD300; kc1, 0x2CFF, in kind
    'c'), k2d00 (SGPR 0x2D00).  Flags E{b}, FA{b}, FD{b}; K{b}, G{b} for the
    products alone.  Kinds 'x' and 'y' are the cold paths (fix_prog,
    prod_fix_prog), whose flags are inputs sE{b}, sFA{b}, sFD{b} / sK{b}, sG{b}."""
    p = "b%d." % b
    U = ["u%d_%d" % (b, i) for i in range(4)]
    V = ["v%d_%d" % (b, i) for i in range(4)]
    prog = []
    E = lambda *a, **k: prog.append(Ins(*a, tag=b, **k))
    if kind == "c":
        canon_prog(E, p, b)
        return prog
    if kind == "x":
        fix_prog(E, p, b)
        return prog
    if kind == "y":
        prod_fix_prog(E, p, b)
        return prog
    if kind == "f":
        W = ["W%d_%d" % (b, j) for j in range(4)]
        X, (tl, th) = fmul_prog(E, p, V, W)
        fold_add_prog(E, p, X, tl, th, ["d%d_%d" % (b, i) for i in range(4)], b)
        return prog
    if kind in ("m", "p"):
        B = [["B%d_%d%d" % (b, k, j) for j in range(4)] for k in range(4)]
        r, T = product_prog(E, p, V, B, kind == "p")
        if kind == "p":
            # s = r + T*C written straight into v (tied output d).  r3 is the
            # low half of a physical register pair, so limb 3 needs an
            # instruction to reach its operand whatever it does: the add keeps
            # its carry into limb 3 (K: the carry out of 2^128, ~2^-48)
            fold_add_prog(E, p, r, T[0], T[1], ["d%d_%d" % (b, i) for i in range(4)], b)
            return prog
        # limb 3 of s is r3 itself; E: the carry that did not reach it
        S = [p + "s%d" % i for i in range(3)] + [r[3]]
        E("add", S[0], [r[0], p + "x0"], sdst=p + "e0")
        E("addc", S[1], [r[1], p + "x1"], sdst=p + "e1", cin=p + "e0")
        E("addc", S[2], [r[2], p + "x2"], sdst="E%d" % b, cin=p + "e1")
    else:
        S = V
    aout = ["a%d_%d" % (b, i) for i in range(4)]  # tied to U
    dout = ["d%d_%d" % (b, i) for i in range(4)]  # tied to V
    if kind == "t":
        # u + v and u - v both read u and v, so whichever comes first cannot
        # overwrite either: limbs 2 and 3 of a go to operands of their own
        aout[2:] = ["x%d_%d" % (b, i) for i in (2, 3)]
    # limbs 0 and 1 wait for the wrap correction; limbs 2 and 3 are final
    A = [p + "A0", p + "A1", aout[2], aout[3]]
    D = [p + "D0", p + "D1", dout[2], dout[3]]
    E("add", A[0], [U[0], S[0]], sdst=p + "f0")
    E("sub", D[0], [U[0], S[0]], sdst=p + "g0")
    for i in (1, 2, 3):
        E("addc", A[i], [U[i], S[i]], sdst=p + ("f%d" % i if i < 3 else "C1"), cin=p + "f%d" % (i - 1))
        E("subb", D[i], [U[i], S[i]], sdst=p + ("g%d" % i if i < 3 else "B1"), cin=p + "g%d" % (i - 1))
    # a + C1*C, d - B1*C on limbs 0 and 1 only, C = 0x2D00*2^32 - 1: the - 1 is
    # the wrap flag itself taken as a borrow-in (carry-in on the d side), and
    # the 0x2D00 goes into limb 1 as minus its negative, so each side is two
    # carry instructions and one select.  Limb 1 carried out (borrowed, for d)
    # exactly when the wrap flag is set and the second instruction's
    # borrow-out (carry-out) is clear: one SALU and-not per side.
    E("subb", aout[0], [A[0], 0], sdst=p + "h0", cin=p + "C1")
    E("addc", dout[0], [D[0], 0], sdst=p + "i0", cin=p + "B1")
    E("cnd", p + "ma", [0, "kneg"], cin=p + "C1")
    E("cnd", p + "md", [0, "kneg"], cin=p + "B1")
    E("subb", aout[1], [A[1], p + "ma"], sdst=p + "h1", cin=p + "h0")
    E("addc", dout[1], [D[1], p + "md"], sdst=p + "i1", cin=p + "i0")
    E("sandn2", None, [], sdst="FA%d" % b, sin=[p + "C1", p + "h1"])
    E("sandn2", None, [], sdst="FD%d" % b, sin=[p + "B1", p + "i1"])
    return prog


# ------------------------------------------------------------- scheduling ---

SGPR_GAP = 3  # consumer index - producer index >= 3: two wait states between
# A SALU read of an SGPR pair that a VALU wrote needs no wait state on gfx950:
# the manual wait-state table of the CDNA3/CDNA4 ISA lists VALU-written SGPRs
# only against VALU (2), VMEM (5) and v_readlane/v_writelane lane-select (4)
# readers, and the SALU interlocks on its own (hipcc itself emits
# v_cmp -> s_and_b64 back to back).  Nor does a VALU read of a SALU-written
# SGPR need one.
SALU_GAP = 1


def schedule(progs, in_order=False):
    """in_order: program order, padded where a dependency asks for it.  Otherwise list-schedule the union of independent instruction lists.  Dependencies:
    true (RAW) on VGPRs (no gap) and SGPRs (SGPR_GAP), plus program order
    between writes/reads of tied output operands.  Priority: longest path."""
    ins = [i for p in progs for i in p]
    n = len(ins)
    writer = {}
    deps = [[] for _ in range(n)]  # (pred, gap)
    readers = {}
    for idx, it in enumerate(ins):
        for r in it.vreads():
            if r in writer:
                deps[idx].append((writer[r], 1))
            readers.setdefault(r, []).append(idx)
        for r in it.sreads():
            if r in writer:  # (not a flag handed in as an operand)
                deps[idx].append((writer[r], SALU_GAP if it.is_salu() or ins[writer[r]].is_salu() else SGPR_GAP))
        for w in it.vwrites() + it.swrites():
            writer[w] = idx
    # tied outputs: a{b}_i overwrites u{b}_i, d{b}_i overwrites v{b}_i -> after every read
    for idx, it in enumerate(ins):
        for w in it.vwrites():
            if w[0] in "ad" and "_" in w and not w.startswith("b"):
                src = ("u" if w[0] == "a" else "v") + w[1:]
                for rd in readers.get(src, []):
                    if rd != idx:
                        deps[idx].append((rd, 0))
    for idx, it in enumerate(ins):
        for nm in it.after:
            for rd in readers.get(nm, []):
                deps[idx].append((rd, 0))
            if nm in writer:
                deps[idx].append((writer[nm], 0))
    succ = [[] for _ in range(n)]
    for i in range(n):
        for (p, g) in deps[i]:
            succ[p].append((i, g))
    prio = [0] * n
    for i in reversed(range(n)):
        prio[i] = 1 + max([prio[s] + (g - 1 if g > 1 else 0) for s, g in succ[i]] + [0])
    done_at = {}
    order = []  # list of instruction indices or None (s_nop 0)
    remaining = set(range(n))
    t = 0
    while remaining:
        ready = [i for i in ([min(remaining)] if in_order else remaining) if all(p in done_at and t - done_at[p] >= g for p, g in deps[i])]
        if not ready:
            order.append(None)
            t += 1
            continue
        # prefer mads slightly (long latency), then priority, then program order
        i = max(ready, key=lambda i: (prio[i], -i))
        order.append(i)
        done_at[i] = t
        remaining.discard(i)
        t += 1
    return ins, order


# -------------------------------------------------------- register alloc ---


def allocate(ins, order):
    """Physical VGPRs for temporaries (pairs even-aligned), SGPR-pair slots for
    carries.  Operand-backed names (inputs/outputs/constants) are not allocated."""
    seq = [ins[i] if i is not None else None for i in order]
    first, last = {}, {}
    pairs = []
    for t, it in enumerate(seq):
        if it is None:
            continue
        for r in it.vreads() + it.sreads():
            last[r] = t
        for w in it.vwrites() + it.swrites():
            first.setdefault(w, t)
            last.setdefault(w, t)
        if isinstance(it.dst, tuple):
            pairs.append((it.dst[1], it.dst[2]))
        for s in it.src:
            if isinstance(s, tuple):
                pairs.append((s[1], s[2]))
    is_temp = lambda r: r.startswith("b") and "." in r
    # pair groups (halves may be defined by different instructions); a lo may
    # have several hi partners with disjoint lifetimes (one odd register)
    lo_his, hi_lo = {}, {}
    for lo, hi in pairs:
        lo_his.setdefault(lo, [])
        if hi not in lo_his[lo]:
            lo_his[lo].append(hi)
        assert hi_lo.get(hi, lo) == lo, ("hi with two lo partners", hi)
        hi_lo[hi] = lo
    vtemps = [r for r in first if is_temp(r) and not is_sgpr_name(r)]
    stemps = [r for r in first if is_temp(r) and is_sgpr_name(r)]
    # half-step intervals: defined by instruction t -> occupied from 2t+1, last
    # read by t -> until 2t, so the reader of a dying value may write the same
    # register (reads precede writes); a dead write still occupies 2t+1
    busy = {}  # phys -> list of (a, b) inclusive

    def span(r):
        return (2 * first[r] + 1, max(2 * last[r], 2 * first[r] + 1))

    def free(phys, a, b):
        for (x, y) in busy.get(phys, []):
            if not (b < x or y < a):
                return False
        return True

    assign = {}
    for r in sorted(vtemps, key=lambda r: first[r]):
        if r in assign:
            continue
        if r in lo_his or r in hi_lo:
            lo = r if r in lo_his else hi_lo[r]
            his = lo_his[lo]
            ivs = [span(h) for h in his]
            for i in range(len(ivs)):
                for j in range(i):
                    a, b = ivs[i], ivs[j]
                    assert a[1] < b[0] or b[1] < a[0], ("hi partners overlap", lo, his)
            ia = span(lo)
            m = 0
            while not (free(VBASE + 2 * m, *ia) and all(free(VBASE + 2 * m + 1, *iv) for iv in ivs)):
                m += 1
            busy.setdefault(VBASE + 2 * m, []).append(ia)
            assign[lo] = "v%d" % (VBASE + 2 * m)
            for h, iv in zip(his, ivs):
                busy.setdefault(VBASE + 2 * m + 1, []).append(iv)
                assign[h] = "v%d" % (VBASE + 2 * m + 1)
        else:
            iv = span(r)
            m = VBASE
            while not free(m, *iv):
                m += 1
            busy.setdefault(m, []).append(iv)
            assign[r] = "v%d" % m
    sbusy = {}
    for r in sorted(stemps, key=lambda r: first[r]):
        iv = span(r)
        m = 0
        while any(not (iv[1] < x or y < iv[0]) for (x, y) in sbusy.get(m, [])):
            m += 1
        sbusy.setdefault(m, []).append(iv)
        assign[r] = ("sgpr", m)
    nv = 1 + max([int(v[1:]) for v in assign.values() if isinstance(v, str)] + [-1])
    ns = 1 + max([v[1] for v in assign.values() if isinstance(v, tuple)] + [-1])
    return seq, assign, nv, ns


def is_sgpr_name(r):
    base = r.split(".", 1)[1]
    return base.startswith(("cy", "bb", "e", "f", "g", "h", "i")) or base in ("C1", "B1")


# ----------------------------------------------------------------- emit ----


def emit(kinds, bsrc):
    """kinds: tuple of 'm' (with twiddle) / 't' (trivial, w = 1) per butterfly.
    bsrc: 's' (twiddle limbs in SGPRs) or 'v'.  Returns (asm lines, operand
    description, nvgpr, nsgpr-pairs)."""
    progs = [bfly_prog(b, k) for b, k in enumerate(kinds)]
    ins, order = schedule(progs, in_order=kinds[0] in "xy")
    seq, assign, nv, ns = allocate(ins, order)
    # trailing pad: the C++ code may read the flag SGPRs with a VALU right away
    # (the flags a SALU instruction wrote need none)
    tail = 0
    for back, it in enumerate(reversed(seq)):
        if it is not None and not it.is_salu() and any(s.startswith(("K", "G", "E", "FA", "FD")) for s in it.swrites()):
            tail = max(tail, SGPR_GAP - 1 - back)
    return seq, assign, nv, ns, max(tail, 0)


def has_u(k):
    return k in ("m", "t", "x")


def operand_names(kinds):
    """outs: tied in/out operands (u{b}_i, v{b}_i) and, for a trivial
    butterfly, the write-only x{b}_2, x{b}_3 (limbs 2, 3 of a).  Its u limbs
    2, 3 are only read but stay in/out operands: a plain input may be given
    the register of another butterfly's in/out operand that holds the same
    value (the zero-padded first pass copies u to v before its second stage),
    and that butterfly overwrites it early."""
    outs, ins = [], []
    for b, k in enumerate(kinds):
        if has_u(k):
            outs += ["u%d_%d" % (b, i) for i in range(4)]
        if k == "t":
            outs += ["x%d_%d" % (b, i) for i in (2, 3)]
        outs += ["v%d_%d" % (b, i) for i in range(4)]
    flags = []
    for b, k in enumerate(kinds):
        if k == "m":
            flags.append("E%d" % b)
        if k in ("p", "f"):
            flags += ["K%d" % b, "G%d" % b]
        if k in ("m", "t"):
            flags += ["FA%d" % b, "FD%d" % b]
    for b, k in enumerate(kinds):
        if k in ("m", "p"):
            ins += ["B%d_%d%d" % (b, kk, j) for kk in range(4) for j in range(4)]
        if k == "f":
            ins += ["W%d_%d" % (b, j) for j in range(4)]
        if k == "x":
            ins += ["sE%d" % b, "sFA%d" % b, "sFD%d" % b]
        if k == "y":
            ins += ["sK%d" % b, "sG%d" % b]
    if any(k in ("m", "t") for k in kinds):
        ins += ["kneg"]
    if any(k == "c" for k in kinds):
        ins += ["kc1"]
    if any(k in ("m", "p", "f") for k in kinds):
        ins += ["k2d00"]
    return outs, flags, ins


def render(kinds, bsrc):
    seq, assign, nv, ns, tail = emit(kinds, bsrc)
    outs, flags, ins = operand_names(kinds)
    # operand numbering: outputs (tied "+v"), flags "=&s", sgpr temps "=&s", junk "=&s", inputs
    opn = {}
    k = 0
    for o in outs:
        opn[o] = k
        k += 1
    for f in flags:
        opn[f] = k
        k += 1
    stmp = []
    for s in range(ns):
        opn[("sgpr", s)] = k
        stmp.append(k)
        k += 1
    opn["junk"] = k
    k += 1
    for i in ins:
        opn[i] = k
        k += 1

    def name(r):
        if isinstance(r, int):
            return str(r)
        if r in assign:
            a = assign[r]
            return "%%%d" % opn[a] if isinstance(a, tuple) else a
        if r[0] in "ad" and "_" in r and "." not in r:  # tied outputs
            return "%%%d" % opn[("u" if r[0] == "a" else "v") + r[1:]]
        return "%%%d" % opn[r]

    def pname(p):
        lo, hi = name(p[1]), name(p[2])
        assert lo.startswith("v") and hi == "v%d" % (int(lo[1:]) + 1) and int(lo[1:]) % 2 == 0, (p, lo, hi)
        return "v[%d:%d]" % (int(lo[1:]), int(hi[1:]))

    lines = []
    for it in seq:
        if it is None:
            lines.append("s_nop 0")
            continue
        # register classes: a temporary's name decides its class (is_sgpr_name)
        for r in it.vreads() + it.vwrites():
            assert not isinstance(assign.get(r), tuple), ("SGPR temporary as a VALU operand", r)
        for r in it.sreads() + it.swrites():
            assert not isinstance(assign.get(r), str), ("VGPR temporary as a mask", r)
        sd = name(it.sdst) if it.sdst else None
        if it.op == "mad":
            s2 = pname(it.src[2]) if isinstance(it.src[2], tuple) else "0"
            lines.append("v_mad_u64_u32 %s, %s, %s, %s, %s" % (pname(it.dst), sd, name(it.src[0]),
                                                               name(it.src[1]), s2))
        elif it.op == "mad24":
            lines.append("v_mad_u32_u24 %s, %s, %s, %s" % (name(it.dst), name(it.src[0]), name(it.src[1]),
                                                          name(it.src[2])))
        elif it.op == "addc":
            lines.append("v_addc_co_u32_e64 %s, %s, %s, %s, %s" % (name(it.dst), sd, name(it.src[0]),
                                                                   name(it.src[1]), name(it.cin)))
        elif it.op == "subb":
            lines.append("v_subb_co_u32_e64 %s, %s, %s, %s, %s" % (name(it.dst), sd, name(it.src[0]),
                                                                   name(it.src[1]), name(it.cin)))
        elif it.op == "add":
            lines.append("v_add_co_u32_e64 %s, %s, %s, %s" % (name(it.dst), sd, name(it.src[0]),
                                                              name(it.src[1])))
        elif it.op == "sub":
            lines.append("v_sub_co_u32_e64 %s, %s, %s, %s" % (name(it.dst), sd, name(it.src[0]),
                                                              name(it.src[1])))
        elif it.op == "cnd":
            lines.append("v_cndmask_b32_e64 %s, %s, %s, %s" % (name(it.dst), name(it.src[0]),
                                                               name(it.src[1]), name(it.cin)))
        elif it.op == "mov":
            lines.append("v_mov_b32 %s, %s" % (name(it.dst), name(it.src[0])))
        elif it.op == "sandn2":
            lines.append("s_andn2_b64 %s, %s, %s" % (sd, name(it.sin[0]), name(it.sin[1])))
        elif it.op == "sor":
            lines.append("s_or_b64 %s, %s, %s" % (sd, name(it.sin[0]), name(it.sin[1])))
        elif it.op == "saveexec":
            lines.append("s_and_saveexec_b64 %s, %s" % (sd, name(it.sin[0])))
        elif it.op == "restexec":
            lines.append("s_mov_b64 exec, %s" % name(it.sin[0]))
        else:
            raise ValueError(it.op)
    if tail:
        lines.append("s_nop %d" % (tail - 1))
    return lines, outs, flags, ins, ns, nv, opn


# ------------------------------------------------------------- emulation ---


def emulate(lines, env):
    """One-lane emulator of the rendered asm.  env maps '%N' operand refs and
    physical 'vN' to 32-bit ints; SGPR pairs to 0/1 carries."""
    regs = dict(env)

    def rd(x):
        if x.startswith("v[") or x.startswith("%") or x.startswith("v"):
            return regs[x]
        return int(x) & MASK32

    def rdp(x):
        if x == "0":
            return 0
        a, b = x[2:-1].split(":")
        return regs["v" + a] | (regs["v" + b] << 32)

    def wrp(x, val):
        a, b = x[2:-1].split(":")
        regs["v" + a] = val & MASK32
        regs["v" + b] = (val >> 32) & MASK32

    for ln in lines:
        op, _, rest = ln.partition(" ")
        a = [s.strip() for s in rest.split(",")] if rest else []
        if op == "s_nop":
            continue
        if op == "s_andn2_b64":
            regs[a[0]] = regs[a[1]] & ~regs[a[2]] & 1
            continue
        if op == "s_or_b64":
            regs[a[0]] = regs[a[1]] | regs[a[2]]
            continue
        if op == "s_and_saveexec_b64":
            # (both operands are read before the destination is written: they may be one pair)
            regs[a[0]], regs["exec"] = regs.get("exec", 1), regs.get("exec", 1) & regs[a[1]]
            continue
        if op == "s_mov_b64":
            assert a[0] == "exec"
            regs["exec"] = regs[a[1]]
            continue
        if not regs.get("exec", 1):
            # an inactive lane: no VGPR write, and a zero bit in a carry-out mask
            if op in ("v_mad_u64_u32", "v_addc_co_u32_e64", "v_add_co_u32_e64", "v_subb_co_u32_e64",
                      "v_sub_co_u32_e64"):
                regs[a[1]] = 0
            continue
        if op == "v_mad_u64_u32":
            v = rd(a[2]) * rd(a[3]) + rdp(a[4])
            wrp(a[0], v)
            regs[a[1]] = v >> 64
        elif op == "v_mad_u32_u24":
            regs[a[0]] = ((rd(a[1]) & 0xFFFFFF) * (rd(a[2]) & 0xFFFFFF) + rd(a[3])) & MASK32
        elif op in ("v_addc_co_u32_e64", "v_add_co_u32_e64"):
            cin = regs[a[4]] if op == "v_addc_co_u32_e64" else 0
            v = rd(a[2]) + rd(a[3]) + cin
            regs[a[0]] = v & MASK32
            regs[a[1]] = v >> 32
        elif op in ("v_subb_co_u32_e64", "v_sub_co_u32_e64"):
            bin_ = regs[a[4]] if op == "v_subb_co_u32_e64" else 0
            v = rd(a[2]) - rd(a[3]) - bin_
            regs[a[0]] = v & MASK32
            regs[a[1]] = 1 if v < 0 else 0
        elif op == "v_cndmask_b32_e64":
            regs[a[0]] = rd(a[2]) if regs[a[3]] else rd(a[1])
        elif op == "v_mov_b32":
            regs[a[0]] = rd(a[1])
        else:
            raise ValueError(op)
    return regs


def check_hazards(lines):
    """Every VALU read of an SGPR written by a VALU must be >= 2 wait states
    later; a SALU read of it, or a read of what a SALU wrote, needs none
    (SALU_GAP)."""
    last_w = {}
    salu_w = set()
    t = 0
    for ln in lines:
        op, _, rest = ln.partition(" ")
        a = [s.strip() for s in rest.split(",")] if rest else []
        if op == "s_nop":
            t += int(a[0]) + 1
            continue
        reads, writes = [], []
        if op in ("v_addc_co_u32_e64", "v_subb_co_u32_e64"):
            reads.append(a[4])
        if op == "v_cndmask_b32_e64":
            reads.append(a[3])
        if op in ("v_mad_u64_u32", "v_addc_co_u32_e64", "v_add_co_u32_e64", "v_subb_co_u32_e64",
                  "v_sub_co_u32_e64"):
            writes.append(a[1])
        salu = op.startswith("s_")
        if op in ("s_andn2_b64", "s_or_b64"):
            reads += [a[1], a[2]]
            writes.append(a[0])
        elif op == "s_and_saveexec_b64":  # (EXEC written by the SALU: no wait state before a VALU)
            reads.append(a[1])
            writes.append(a[0])
        elif op == "s_mov_b64":
            reads.append(a[1])
        elif salu:
            raise ValueError(op)
        for r in reads:
            gap = SALU_GAP if salu or r in salu_w else SGPR_GAP
            if r in last_w and t - last_w[r] < gap:
                raise AssertionError("SGPR hazard on %s at '%s' (distance %d)" % (r, ln, t - last_w[r]))
        for w in writes:
            last_w[w] = t
            (salu_w.add if salu else salu_w.discard)(w)
        t += 1


def limbs(x):
    return [(x >> (32 * i)) & MASK32 for i in range(4)]


def value(l):
    return sum(v << (32 * i) for i, v in enumerate(l))


def run_regs(kinds, lines, opn, uvals, vvals, wvals):
    """Emulate one lane and return the register file: operand N is at '%N'
    (opn maps operand names, flags included, to N)."""
    env = {}
    for b in range(len(kinds)):
        for i in range(4):
            if has_u(kinds[b]):
                env["%%%d" % opn["u%d_%d" % (b, i)]] = limbs(uvals[b])[i]
            env["%%%d" % opn["v%d_%d" % (b, i)]] = limbs(vvals[b])[i]
        if kinds[b] in ("m", "p"):
            Bs = [wvals[b] * (1 << (32 * k)) % M for k in range(4)]
            for k in range(4):
                for j in range(4):
                    env["%%%d" % opn["B%d_%d%d" % (b, k, j)]] = limbs(Bs[k])[j]
        if kinds[b] == "f":
            for j in range(4):
                env["%%%d" % opn["W%d_%d" % (b, j)]] = limbs(wvals[b])[j]
    if "kc1" in opn:
        env["%%%d" % opn["kc1"]] = KC1
    if "kneg" in opn:
        env["%%%d" % opn["kneg"]] = KNEG
    if "k2d00" in opn:
        env["%%%d" % opn["k2d00"]] = K2D00
    return emulate(lines, env)


def run_case(kinds, lines, opn, nv, uvals, vvals, wvals):
    """Emulate one lane; apply the flag fixes as the C++ cold path does;
    return [(a, d)] as integers (a = None for the one-operand kinds)."""
    regs = run_regs(kinds, lines, opn, uvals, vvals, wvals)
    res = []
    for b in range(len(kinds)):
        d = value([regs["%%%d" % opn["v%d_%d" % (b, i)]] for i in range(4)])
        if kinds[b] in ("p", "f"):  # v <- w v; true value d + K 2^128 - G 2^64
            d = relaxed_add(d, regs["%%%d" % opn["K%d" % b]] << 128)
            res.append((None, relaxed_sub(d, regs["%%%d" % opn["G%d" % b]] << 64)))
            continue
        if kinds[b] == "c":
            res.append((None, d))
            continue
        hi = "x" if kinds[b] == "t" else "u"
        a = value([regs["%%%d" % opn["%s%d_%d" % ("u" if i < 2 else hi, b, i)]] for i in range(4)])
        fe = regs["%%%d" % opn["E%d" % b]] if kinds[b] == "m" else 0
        fa = regs["%%%d" % opn["FA%d" % b]]
        fd = regs["%%%d" % opn["FD%d" % b]]
        a, d = fix(a, d, fe, fa, fd)
        res.append((a, d))
    return res


def run_fix(lines, opn, a, d, fe, fa, fd, active=1):
    """Emulate one lane of the fix statement (kind 'x'); active: the lane's
    EXEC bit on entry.  Returns (a, d, EXEC bit on exit)."""
    env = {"exec": active}
    for i in range(4):
        env["%%%d" % opn["u0_%d" % i]] = limbs(a)[i]
        env["%%%d" % opn["v0_%d" % i]] = limbs(d)[i]
    for nm, f in (("sE0", fe), ("sFA0", fa), ("sFD0", fd)):
        env["%%%d" % opn[nm]] = f
    regs = emulate(lines, env)
    return (value([regs["%%%d" % opn["u0_%d" % i]] for i in range(4)]),
            value([regs["%%%d" % opn["v0_%d" % i]] for i in range(4)]), regs["exec"])


def run_prod_fix(lines, opn, v, fk, fg, active=1):
    """As run_fix for the products' statement (kind 'y'): (v, EXEC bit on exit)."""
    env = {"exec": active, "%%%d" % opn["sK0"]: fk, "%%%d" % opn["sG0"]: fg}
    for i in range(4):
        env["%%%d" % opn["v0_%d" % i]] = limbs(v)[i]
    regs = emulate(lines, env)
    return value([regs["%%%d" % opn["v0_%d" % i]] for i in range(4)]), regs["exec"]


def prod_fix(v, fk, fg):
    """The products' cold path (C++ prod_fix): + C for fk, then - 2^64 for fg."""
    return relaxed_sub(relaxed_add(v, fk << 128), fg << 64)


def fix_operands():
    """Operands for the cold-path statements: around 0 and 2^128 at the
    distances the add-backs and their re-wraps turn on (2^64, 2^96, C)."""
    top = (1 << 128) - 1
    out = [0, 1, top, (1 << 64) - 1, 1 << 64, (1 << 96) - 1, 1 << 96, (1 << 96) + (1 << 64) - 1, (1 << 96) + (1 << 64)]
    for base in (0, 1 << 64, 1 << 96, (1 << 96) + (1 << 64), C, 2 * C):
        for off in (-1, 0, 1):
            out += [(top + 1 - base + off) % (1 << 128), (base + off) % (1 << 128)]
    return sorted(set(out))


def fix_selftest(kind, lines, opn, trials=200, seed=3):
    """The cold-path statements against fix() / prod_fix(): every flag
    combination on random and edge operands, active and inactive lanes."""
    rng = random.Random(seed)
    edge = fix_operands()
    n = 0
    for t in range(trials):
        a = rng.choice(edge) if rng.random() < 0.5 else rng.randrange(1 << 128)
        d = rng.choice(edge) if rng.random() < 0.5 else rng.randrange(1 << 128)
        for f in range(8 if kind == "x" else 4):
            fe, fa, fd = f & 1, (f >> 1) & 1, f >> 2
            if kind == "x":
                assert run_fix(lines, opn, a, d, fe, fa, fd) == fix(a, d, fe, fa, fd) + (1,), (a, d, fe, fa, fd)
                assert run_fix(lines, opn, a, d, fe, fa, fd, active=0) == (a, d, 0), (a, d, fe, fa, fd)
            else:
                assert run_prod_fix(lines, opn, d, fe, fa) == (prod_fix(d, fe, fa), 1), (d, fe, fa)
                assert run_prod_fix(lines, opn, d, fe, fa, active=0) == (d, 0), (d, fe, fa)
            n += 1
    return n


def relaxed_add(x, y):
    """x + y in the relaxed representation: a wrap out of 2^128 adds C, and a
    second wrap adds C again."""
    x += y
    for _ in range(2):
        if x >> 128:
            x = (x & ((1 << 128) - 1)) + C
    return x


def relaxed_sub(x, y):
    """x - y in the relaxed representation: a borrow out of 2^128 subtracts C,
    and a second borrow subtracts C again."""
    x -= y
    for _ in range(2):
        if x < 0:
            x = x + (1 << 128) - C
    return x


def fix(a, d, fe, fa, fd):
    """The cold path of the C++ wrapper: the ripples the asm leaves out are
    added back (fa: the carry out of limb 1 of a, fd: the borrow out of limb
    1 of d, fe: the carry out of limb 2 of s = w v, which both a and d miss)."""
    return relaxed_add(a, (fa << 64) + (fe << 96)), relaxed_sub(d, (fd << 64) + (fe << 96))


def model(u, v, w=None):
    """One butterfly as the asm computes it, on integers: (a, d, fe, fa, fd)
    before the cold path; w = None is the trivial butterfly.  fix() of these
    is exact mod M; the flags say which operands reach the cold path."""
    m96, m64 = (1 << 96) - 1, (1 << 64) - 1
    s, fe = v, 0
    if w is not None:
        P = sum(vk * (w * (1 << (32 * k)) % M) for k, vk in enumerate(limbs(v)))
        r = P & ((1 << 128) - 1)
        lo = (r & m96) + (P >> 128) * C
        s, fe = (r & ~m96) | (lo & m96), lo >> 96
    A, D = u + s, u - s
    la = (A & m64) + (A >> 128) * C
    ld = (D & m64) - (C if D < 0 else 0)
    a = (A & ((1 << 128) - 1) & ~m64) | (la & m64)
    d = (D & ((1 << 128) - 1) & ~m64) | (ld & m64)
    return a, d, fe, la >> 64, 1 if ld < 0 else 0


def selftest(kinds, lines, opn, nv, trials=3000, seed=1):
    rng = random.Random(seed)
    edge = [0, 1, M - 1, M, (1 << 128) - 1, C, C - 1, (1 << 128) - C, (1 << 128) - C - 1, M - C,
            (1 << 127), (1 << 96) - 1, 0xFFFFFFFF, ((1 << 128) - 1) ^ 0xFFFFFFFF,
            (1 << 64) - 1, (1 << 64) - C, (1 << 64) - C - 1, 1 << 96]
    # twiddles: roots of unity of small order (what the NTT uses) and random
    roots = []
    g = pow(3, (M - 1) >> 9, M)
    for e in range(512):
        roots.append(pow(g, e, M))
    roots = [w for w in roots if w != M - 1]
    checked = 0
    for t in range(trials):
        nb = len(kinds)
        pick = lambda: rng.choice(edge) if rng.random() < 0.3 else rng.randrange(1 << 128)
        uv = [pick() for _ in range(nb)]
        vv = [pick() for _ in range(nb)]
        # products ('p') take any canonical twiddle, limbs of 0xFFFFFFFF included
        wv = [rng.choice(roots) if k not in ("p", "f") else
              (rng.choice([M - 1, M - 2, (1 << 127) | 0xFFFFFFFF_FFFFFFFF_FFFFFFFF, 1, 2])
               if rng.random() < 0.3 else rng.randrange(M)) for k in kinds]
        got = run_case(kinds, lines, opn, nv, uv, vv, wv)
        for b in range(nb):
            w = wv[b] if kinds[b] in ("m", "p", "f") else 1
            a, d = got[b]
            if kinds[b] in ("p", "f"):
                assert 0 <= d < (1 << 128) and d % M == (w * vv[b]) % M, (kinds, b, vv[b], w)
                checked += 1
                continue
            if kinds[b] == "c":
                assert d == vv[b] % M, (kinds, b, vv[b])
                checked += 1
                continue
            assert 0 <= a < (1 << 128) and 0 <= d < (1 << 128)
            assert a % M == (uv[b] + w * vv[b]) % M, (kinds, b, uv[b], vv[b], w)
            assert d % M == (uv[b] - w * vv[b]) % M, (kinds, b, uv[b], vv[b], w)
            checked += 1
    return checked


def twiddle_precondition():
    """Max of w's limbs 1..3 over all roots of order <= 2^9 except -1."""
    g = pow(3, (M - 1) >> 9, M)
    worst = 0
    for e in range(512):
        w = pow(g, e, M)
        if w == M - 1:
            continue
        worst = max(worst, max(limbs(w)[1:]))
    return worst


# ------------------------------------------------------------ C++ header ---

VARIANTS = [("m", "m"), ("m",), ("t", "t"), ("t",), ("m", "t"), ("p", "p"), ("p",), ("f", "f"), ("f",),
            ("c", "c", "c", "c"), ("c",)]


def cxx_fix(kind):
    """The cold-path statement as a function: kind 'x' bfly_fix_asm, 'y' prod_fix_asm."""
    lines, outs, flags, ins, ns, nv, opn = render((kind,), "v")
    assert not flags
    cname = {"u": "a", "v": "d" if kind == "x" else "v"}
    ol = ['"+v"(%s.w[%s])' % (cname[o[0]], o.split("_")[1]) for o in outs]
    ol += ['"=&s"(st[%d])' % s for s in range(ns)] + ['"=&s"(junk)']
    arg = {"sE0": "fe_", "sFA0": "fa", "sFD0": "fd", "sK0": "fk", "sG0": "fg"}
    il = ['"s"(%s)' % arg[i] for i in ins]
    clob = ", ".join(['"v%d"' % (VBASE + r) for r in range(nv)] + ['"scc"'])
    stats = "%d VALU, %d s_nop, %d VGPR temps, %d SGPR-pair temps" % (
        sum(1 for l in lines if l.startswith("v_")), sum(1 for l in lines if l.startswith("s_nop")), nv, ns)
    head = ("bfly_fix_asm(fe& a, fe& d, uint64_t fe_, uint64_t fa, uint64_t fd)" if kind == "x" else
            "prod_fix_asm(fe& v, uint64_t fk, uint64_t fg)")
    code = ("// %s as one statement, on the lanes a flag names: the limbs are in/out\n"
            "// operands, so the rare-case block leaves them in the registers they have.\n// %s\n"
            "__device__ __forceinline__ void %s {\n"
            "  uint64_t st[%d];\n  uint64_t junk;\n"
            '  asm volatile(\n      "%s"\n      : %s\n      : %s\n      : %s);\n}\n') % (
        "bfly_fix" if kind == "x" else "prod_fix", stats, head, ns, "\\n\\t".join(lines), ",\n        ".join(ol),
        ",\n        ".join(il), clob)
    return code, lines, opn


def cxx_function(kinds, bsrc):
    lines, outs, flags, ins, ns, nv, opn = render(kinds, bsrc)
    fname = "bfly_%s_%s" % ("".join(kinds), bsrc)
    nb = len(kinds)
    args = []
    for b in range(nb):
        args += (["fe& u%d" % b] if has_u(kinds[b]) else []) + ["fe& v%d" % b]
        if kinds[b] in ("m", "p"):
            args += ["const fe& B%d_%d" % (b, k) for k in range(4)]
        if kinds[b] == "f":
            args.append("const fe& W%d" % b)
    # the corrections' constant: a parameter, so that a kernel holds it in one
    # VGPR for all its statements; the overload without it passes the literal
    kconst = [(k, v) for k, v in (("kneg", KNEG), ("kc1", KC1)) if k in ins]
    thin_args = list(args)
    args += ["uint32_t %s" % k for k, _ in kconst]
    if flags:
        args += ["uint64_t& rare"]
        thin_args += ["uint64_t& rare"]
    body = []
    for f in flags:
        body.append("  uint64_t %s;" % f)
    for o in outs:
        if o[0] == "x":
            body.append("  uint32_t %s;" % o)
    if ns:
        body.append("  uint64_t st[%d];" % ns)
    body.append("  uint64_t junk;")
    if "k2d00" in ins:
        body.append("  const uint32_t k2d00 = 0x2D00u;")
    asm = "\\n\\t".join(lines)
    ol = []
    for o in outs:
        b, i = o[1:].split("_")
        ol.append('"=&v"(%s)' % o if o[0] == "x" else '"+v"(%s%s.w[%s])' % (o[0], b, i))
    for f in flags:
        ol.append('"=&s"(%s)' % f)
    for s in range(ns):
        ol.append('"=&s"(st[%d])' % s)
    ol.append('"=&s"(junk)')
    il = []
    for i in ins:
        if i in ("kc1", "kneg"):
            il.append('"v"(%s)' % i)
        elif i == "k2d00":
            il.append('"s"(k2d00)')
        elif i[0] == "W":
            b, j = i[1:].split("_")
            il.append('"v"(W%s.w[%s])' % (b, j))
        else:
            b, kj = i[1:].split("_")
            il.append('"%s"(B%s_%s.w[%s])' % (bsrc, b, kj[0], kj[1]))
    clob = ", ".join(['"v%d"' % (VBASE + r) for r in range(nv)] +
                     (['"scc"'] if any(l.startswith("s_andn2") for l in lines) else []))
    body.append('  asm volatile(\n      "%s"\n      : %s\n      : %s\n      : %s);' % (
        asm, ",\n        ".join(ol), ",\n        ".join(il), clob))
    for o in outs:
        if o[0] == "x":
            b, i = o[1:].split("_")
            body.append("  u%s.w[%s] = %s;" % (b, i, o))
    if flags:
        body.append("  rare = %s;" % " | ".join(flags))
        body.append("  if (__builtin_expect(rare != 0, 0)) {")
    for b in range(nb):
        if kinds[b] in ("p", "f"):
            body.append("    prod_fix_asm(v%d, K%d, G%d);" % (b, b, b))
        elif kinds[b] != "c":
            fe = "E%d" % b if kinds[b] == "m" else "0ull"
            body.append("    bfly_fix_asm(u%d, v%d, %s, FA%d, FD%d);" % (b, b, fe, b, b))
    if flags:
        body.append("  }")
    stats = "%d VALU, %d s_nop, %d VGPR temps, %d SGPR-pair temps" % (
        sum(1 for l in lines if l.startswith("v_")), sum(1 for l in lines if l.startswith("s_nop")), nv, ns)
    code = "// %s\n__device__ __forceinline__ void %s(%s) {\n%s\n}\n" % (
        stats, fname, ", ".join(args), "\n".join(body))
    if kconst:
        call = [a.split()[-1] for a in thin_args]
        call[len(call) - (1 if flags else 0):len(call) - (1 if flags else 0)] = ["0x%Xu" % v for _, v in kconst]
        code += "__device__ __forceinline__ void %s(%s) {\n  %s(%s);\n}\n" % (
            fname, ", ".join(thin_args), fname, ", ".join(call))
    return fname, code, lines


HEADER = """// GENERATED by tools/gen_bfly.py -- do not edit by hand.
//
// Hand-scheduled gfx950 radix-2 DIT butterflies over F_M in the relaxed
// representation (any residue in [0, 2^128)); see tools/gen_bfly.py for the
// algorithm, the hazard rule they are scheduled for and the emulator that
// checks them (tests/test_bfly_asm.py).  (u, v) -> (u + w v, u - w v), w given
// as its expanded multiples B_k = w 2^(32k) mod M (stage twiddle tables).
// Temporaries use physical VGPRs v0..; the statements clobber them.
#pragma once
#include "field.hpp"

namespace mlh {

// Relaxed x + C / x - C (one wrap corrected; the second cannot wrap).
__device__ __forceinline__ fe relaxed_add_c(const fe& x) {
  uint32_t k;
  fe t = add_c(x, &k);
  if (k) {
    uint32_t k2;
    t = add_c(t, &k2);
  }
  return t;
}
__device__ __forceinline__ fe relaxed_sub_c(const fe& x) {
  fe t;
  uint32_t b;
  t.w[0] = subb(x.w[0], kC0, 0u, &b);
  t.w[1] = subb(x.w[1], kC1, b, &b);
  t.w[2] = subb(x.w[2], 0u, b, &b);
  t.w[3] = subb(x.w[3], 0u, b, &b);
  if (b) {
    t.w[0] = subb(t.w[0], kC0, 0u, &b);
    t.w[1] = subb(t.w[1], kC1, b, &b);
    t.w[2] = subb(t.w[2], 0u, b, &b);
    t.w[3] = subb(t.w[3], 0u, b, &b);
  }
  return t;
}

// Relaxed x + y / x - y: a wrap out of 2^128 is worth C (2^128 = C mod M), and
// adding or subtracting that C may wrap once more.
__device__ __forceinline__ fe relaxed_add(const fe& x, const fe& y) {
  fe t;
  uint32_t k;
  t.w[0] = addc(x.w[0], y.w[0], 0u, &k);
  t.w[1] = addc(x.w[1], y.w[1], k, &k);
  t.w[2] = addc(x.w[2], y.w[2], k, &k);
  t.w[3] = addc(x.w[3], y.w[3], k, &k);
  return k ? relaxed_add_c(t) : t;
}
__device__ __forceinline__ fe relaxed_sub(const fe& x, const fe& y) {
  fe t;
  uint32_t b;
  t.w[0] = subb(x.w[0], y.w[0], 0u, &b);
  t.w[1] = subb(x.w[1], y.w[1], b, &b);
  t.w[2] = subb(x.w[2], y.w[2], b, &b);
  t.w[3] = subb(x.w[3], y.w[3], b, &b);
  return b ? relaxed_sub_c(t) : t;
}

// Cold path in plain C++: what the generated bfly_fix_asm / prod_fix_asm below
// compute (the wrappers call those).  The butterflies leave out the carry
// ripples that are almost never set and flag the lanes where one was: fa, the carry out of limb 1 of
// a when it took its + C (true a = a + 2^64); fd, the borrow out of limb 1 of
// d when it took its - C (true d = d - 2^64); fe, the carry out of limb 2 of
// s = w v when the top word was folded in (true s = s + 2^96, which a gains
// and d loses).
__device__ __forceinline__ void bfly_fix_lane(fe& a, fe& d, uint32_t fe_, uint32_t fa, uint32_t fd) {
  a = relaxed_add(a, fe{{0u, 0u, fa, fe_}});
  d = relaxed_sub(d, fe{{0u, 0u, fd, fe_}});
}
__device__ __forceinline__ void bfly_fix(fe& a, fe& d, uint64_t fe_, uint64_t fa, uint64_t fd) {
  const uint32_t lane = __lane_id();
  bfly_fix_lane(a, d, (uint32_t)(fe_ >> lane) & 1u, (uint32_t)(fa >> lane) & 1u, (uint32_t)(fd >> lane) & 1u);
}

// Products alone (v <- w v): fk, the sum carried out of 2^128 (true v = v + C);
// fg, the borrow out of limb 1 that the fold's - T left out (true v = v - 2^64).
__device__ __forceinline__ void prod_fix(fe& v, uint64_t fk, uint64_t fg) {
  const uint32_t lane = __lane_id();
  if ((fk >> lane) & 1u) v = relaxed_add_c(v);
  if ((fg >> lane) & 1u) v = relaxed_sub(v, fe{{0u, 0u, 1u, 0u}});
}

// Canonical representative of a relaxed value (x < 2^128 < 2M).
__device__ __forceinline__ fe relaxed_canon(const fe& x) { return canon_with_carry(x, 0u); }

"""


def main():
    parts = [HEADER]
    total = 0
    for kind in "xy":
        code, lines, opn = cxx_fix(kind)
        check_hazards(lines)
        total += fix_selftest(kind, lines, opn)
        parts.append(code)
    for kinds in VARIANTS:
        for bsrc in ("s", "v"):
            if not any(k in ("m", "p") for k in kinds) and bsrc == "s":
                continue
            fname, code, lines = cxx_function(kinds, bsrc)
            _, _, _, _, _, nv, opn = render(kinds, bsrc)
            check_hazards(lines)
            total += selftest(kinds, lines, opn, nv, trials=400)
            parts.append(code)
    parts.append("}  // namespace mlh\n")
    open(OUT, "w").write("\n".join(parts))
    print("wrote", OUT, "emulated butterflies:", total, "twiddle max limb:", hex(twiddle_precondition()))


if __name__ == "__main__":
    main()
