"""Seeded generators of constraint programs and fill programs, each with a
reference that shares nothing with the code under test, for
tests/test_program_fuzz_cpu.py and tests/test_program_fuzz_gpu.py.

  expr_case(seed)    random expression trees (CS.Expr) of bounded degree and,
                     built in the same recursion, plain closures f(row, randoms)
                     -> int, the form tests/cs_reference.py takes
  instr_case(seed)   random instruction lists over the wire format, operand
                     forms the compiler never emits among them; the reference
                     interprets the generator's own tuples with Python integers
                     and keeps its own formal degrees
  fill_case(seed)    both levels for fill programs (compile_fill with CS.inv,
                     and raw instructions), with its own inverse-taint book

CS_TABLE and FILL_TABLE are the committed cases: every entry must build and run
(the CPU test asserts what the table covers, so an edit cannot hollow it out).
"""
import random

from multilinear_amd import constraint_system as CS
from oracle import field as F

M = F.M
ADD, SUB, MUL, NEG, INV = range(5)
COL, RAND, CONST, TEMP = range(4)
EDGES = [0, 1, M - 1, M - 2, 2 ** 64, 2 ** 96 - 1]


def _const(r):
    """0, 1, 2, M - 1 or a random element (half the time: a zero factor makes
    what it multiplies dead code)."""
    return r.choice([0, 1, 2, M - 1] + 4 * [r.randrange(M)])


def matrix(seed, height, width):
    """Random canonical elements; about one row in eight from EDGES."""
    r = random.Random("matrix %s %d %d" % (seed, height, width))
    out = []
    for _ in range(height):
        if r.randrange(8) == 0:
            out += [r.choice(EDGES) for _ in range(width)]
        else:
            out += [r.randrange(M) for _ in range(width)]
    return out


def elements(seed, n):
    r = random.Random("elements %s" % (seed,))
    return [r.randrange(M) for _ in range(n)]


# ---- expression level ----------------------------------------------------------

class _ExprGen:
    """Trees by recursive descent; a `mul` splits the degree budget between its
    operands.  Every node is (Expr, closure, formal degree)."""

    def __init__(self, r, width, n_randoms, max_depth, dag=False, nxt=False, no_col=None):
        self.r, self.W, self.NR, self.max_depth = r, width, n_randoms, max_depth
        self.dag, self.nxt, self.no_col = dag, nxt, no_col
        self.pool = []     # subtrees built so far (a DAG reuses the objects)
        self.shifts = []   # nxt columns in order of first appearance
        self.shared = 0

    def leaf(self, deg):
        r, k = self.r, self.r.random()
        cols = [j for j in range(self.W) if j != self.no_col]
        if k < 0.6 and deg >= 1 and cols:
            j = r.choice(cols)
            if self.nxt and r.random() < 0.4:
                if j not in self.shifts:
                    self.shifts.append(j)
                p = self.W + self.shifts.index(j)  # its column of the extended row
                return CS.nxt(j), (lambda x, rn, p=p: x[p]), 1
            return CS.var(j), (lambda x, rn, j=j: x[j]), 1
        if k < 0.8 and self.NR:
            j = r.randrange(self.NR)
            return CS.rand(j), (lambda x, rn, j=j: rn[j]), 0
        c = _const(r)
        return CS.const(c), (lambda x, rn, c=c: c), 0

    def tree(self, deg, depth=0):
        r = self.r
        if self.dag and self.pool and r.random() < 0.2:
            fit = [n for n in self.pool if n[2] <= deg]
            if fit:
                self.shared += 1
                return r.choice(fit)
        if depth >= self.max_depth or r.random() < 0.15:
            return self.leaf(deg)
        op = r.choice(["add", "sub", "mul", "mul", "neg"])
        if op == "neg":
            e, f, d = self.tree(deg, depth + 1)
            node = (-e, (lambda x, rn, f=f: (-f(x, rn)) % M), d)
        elif op == "mul":
            a, fa, d1 = self.tree(r.randint(0, deg), depth + 1)
            b, fb, d2 = self.tree(deg - d1, depth + 1)
            node = (a * b, (lambda x, rn, fa=fa, fb=fb: fa(x, rn) * fb(x, rn) % M), d1 + d2)
        else:
            a, fa, d1 = self.tree(deg, depth + 1)
            b, fb, d2 = self.tree(deg, depth + 1)
            if op == "add":
                node = (a + b, (lambda x, rn, fa=fa, fb=fb: (fa(x, rn) + fb(x, rn)) % M), max(d1, d2))
            else:
                node = (a - b, (lambda x, rn, fa=fa, fb=fb: (fa(x, rn) - fb(x, rn)) % M), max(d1, d2))
        self.pool.append(node)
        return node


class CsCase:
    """A constraint program with its reference.  fns: callables f(row, randoms)
    -> int per constraint; formal: the formal degree by the generator's own
    book; degree: the declared one.  Instruction level: consts, n_temps,
    instrs, outs as given to encode_program."""

    level = None
    consts = instrs = outs = None
    n_temps = 0
    shifts = ()
    shared = 0

    def __init__(self, level, seed, width, n_randoms, degree, formal, fns):
        self.level, self.seed, self.width, self.n_randoms = level, seed, width, n_randoms
        self.degree, self.formal, self.fns = degree, formal, fns
        self.n_constraints = len(fns)

    def composition(self, row, randoms, mask):
        return sum(mk * f(row, randoms) for f, mk in zip(self.fns, mask)) % M


def _budget(r, degree):
    """The degree the generator aims at: a pinned declared degree itself half the time."""
    if degree is not None and r.random() < 0.5:
        return degree
    return r.randint(1, degree if degree is not None else 7)


def _declared(r, formal, degree):
    if degree is not None:
        return degree
    return formal if r.random() < 0.6 else r.randint(formal, 7)


def expr_case(seed, width=None, n_randoms=None, n_constraints=None, degree=None, nxt=False):
    """Random expression trees compiled by compile_program (compile_shifted with
    nxt=True: `wire` then has width + len(shifts) columns and the closures read
    the extended row).  degree pins the declared degree."""
    r = random.Random("expr %d" % seed)
    W = width if width is not None else r.randint(1, 32)
    NR = n_randoms if n_randoms is not None else r.randint(0, 4)
    nc = n_constraints if n_constraints is not None else r.randint(1, 6)
    budget = _budget(r, degree)
    g = _ExprGen(r, W, NR, r.randint(2, 6), dag=r.random() < 0.4, nxt=nxt)
    nodes = [g.tree(budget) for _ in range(nc)]
    if max(n[2] for n in nodes) == 0:  # a composition of degree 0 has no declared degree
        j = r.randrange(W)
        nodes[r.randrange(nc)] = (CS.var(j), (lambda x, rn, j=j: x[j]), 1)
    formal = max(n[2] for n in nodes)
    case = CsCase("expr", seed, W, NR, _declared(r, formal, degree), formal, [n[1] for n in nodes])
    case.exprs = [n[0] for n in nodes]
    case.shared = g.shared
    if nxt:
        case.shifts = list(g.shifts)
        case.wire, case.got_shifts = CS.compile_shifted(case.exprs, W, NR, case.degree)
    else:
        case.wire = CS.compile_program(case.exprs, W, NR, case.degree)
    return case


# ---- instruction level -----------------------------------------------------------

class _Interp:
    """The generator's instruction tuples on Python integers (INV: x^(M-2), so
    zero gives zero).  One run per (row, randoms) serves every output."""

    def __init__(self, width, n_randoms, consts, n_temps, instrs):
        self.W, self.NR, self.consts, self.T = width, n_randoms, list(consts), n_temps
        off = (0, width, width + n_randoms, width + n_randoms + len(consts))
        self.off = off
        self.code = [(op, off[TEMP] + dst, off[a[0]] + a[1], off[b[0]] + b[1])
                     for op, dst, a, b in instrs]
        self.key = self.env = None

    def run(self, row, randoms, stop=None):
        """The environment [row | randoms | consts | temps] after the first
        `stop` instructions (all of them by default)."""
        e = list(row[:self.W]) + list(randoms[:self.NR]) + self.consts + [0] * self.T
        for op, d, a, b in (self.code if stop is None else self.code[:stop]):
            if op == MUL:
                e[d] = e[a] * e[b] % M
            elif op == ADD:
                e[d] = (e[a] + e[b]) % M
            elif op == SUB:
                e[d] = (e[a] - e[b]) % M
            elif op == NEG:
                e[d] = -e[a] % M
            else:
                e[d] = pow(e[a], M - 2, M)
        return e

    def operand(self, row, randoms, o):
        key = (tuple(row), tuple(randoms))
        if key != self.key:
            self.env, self.key = self.run(row, randoms), key
        return self.env[self.off[o[0]] + o[1]]


class _CodeGen:
    """Random straight-line code.  Its own book per temp value: formal degree
    (None: never written), inverse taint, the columns the value depends on."""

    def __init__(self, r, width, n_randoms, n_consts, n_temps, max_degree):
        self.r, self.W, self.NR, self.NC, self.T, self.maxdeg = (r, width, n_randoms, n_consts,
                                                                  n_temps, max_degree)
        self.deg = [None] * n_temps
        self.taint = [False] * n_temps
        self.cols = [set() for _ in range(n_temps)]
        self.instrs = []
        self.reserved = None  # a temp dst() never picks

    def written(self, tainted=None):
        return [t for t in range(self.T) if self.deg[t] is not None
                and (tainted is None or self.taint[t] == tainted)]

    def operand(self, tainted=None, avoid=None):
        """(kind, index); tainted=False: no value that depends on an INV;
        avoid: a column the value must not depend on."""
        r = self.r
        kinds = [COL] * 3 if self.W > (1 if avoid is not None else 0) else []
        kinds += [RAND] * 2 * bool(self.NR) + [CONST] * 2 * bool(self.NC)
        temps = [t for t in self.written(tainted) if avoid is None or avoid not in self.cols[t]]
        kinds += [TEMP] * 5 * bool(temps)
        k = r.choice(kinds)
        if k == COL:
            return (COL, r.choice([j for j in range(self.W) if j != avoid]))
        if k == RAND:
            return (RAND, r.randrange(self.NR))
        if k == CONST:
            return (CONST, r.randrange(self.NC))
        return (TEMP, r.choice(temps))

    def odeg(self, o):
        return 1 if o[0] == COL else (self.deg[o[1]] if o[0] == TEMP else 0)

    def otaint(self, o):
        return o[0] == TEMP and self.taint[o[1]]

    def ocols(self, o):
        return {o[1]} if o[0] == COL else (set(self.cols[o[1]]) if o[0] == TEMP else set())

    def emit(self, op, dst, a, b=(0, 0)):
        if op in (NEG, INV):
            d, t, c = self.odeg(a), self.otaint(a) or op == INV, self.ocols(a)
        else:
            da, db = self.odeg(a), self.odeg(b)
            d = da + db if op == MUL else max(da, db)
            t, c = self.otaint(a) or self.otaint(b), self.ocols(a) | self.ocols(b)
        self.deg[dst], self.taint[dst], self.cols[dst] = d, t, c
        self.instrs.append((op, dst, a, b))

    def dst(self, a, b):
        r, k = self.r, self.r.random()
        if k < 0.2 and a[0] == TEMP:
            return a[1]
        if k < 0.35 and b[0] == TEMP:
            return b[1]
        return r.choice([t for t in range(self.T) if t != self.reserved])

    def arith(self, tainted=None):
        """One ADD / SUB / MUL / NEG; a MUL above the degree budget becomes an ADD."""
        r = self.r
        op = r.choice([ADD, SUB, MUL, MUL, NEG])
        a = self.operand(tainted)
        if op == NEG:
            return self.emit(NEG, self.dst(a, (COL, 0)), a)
        b = a if (a[0] == TEMP and r.random() < 0.15) else self.operand(tainted)
        if op == MUL and self.odeg(a) + self.odeg(b) > self.maxdeg:
            op = r.choice([ADD, SUB])
        self.emit(op, self.dst(a, b), a, b)


def _pick(r, value, lo, hi):
    return value if value is not None else r.randint(lo, hi)


def instr_case(seed, width=None, n_randoms=None, n_consts=None, n_temps=None, n_instr=None,
               n_constraints=None, degree=None):
    """A random constraint program in raw instructions (encode_program).
    degree pins the declared degree."""
    r = random.Random("instr %d" % seed)
    W = _pick(r, width, 1, 32)
    NR, NC = _pick(r, n_randoms, 0, 5), _pick(r, n_consts, 0, 5)
    T = _pick(r, n_temps, 1, 12)
    n = _pick(r, n_instr, 4, 80)
    nc = _pick(r, n_constraints, 1, 9)
    g = _CodeGen(r, W, NR, NC, T, _budget(r, degree))
    consts = [_const(r) for _ in range(NC)]
    for _ in range(n):
        g.arith()
    outs = []
    for _ in range(nc):
        k = r.random()
        if k < 0.7 and g.written():
            outs.append((TEMP, r.choice(g.written())))
        else:
            outs.append(g.operand())
    if max(g.odeg(o) for o in outs) == 0:
        outs[r.randrange(nc)] = (COL, r.randrange(W))
    formal = max(g.odeg(o) for o in outs)
    ref = _Interp(W, NR, consts, T, g.instrs)
    fns = [(lambda x, rn, o=o: ref.operand(x, rn, o)) for o in outs]
    case = CsCase("instr", seed, W, NR, _declared(r, formal, degree), formal, fns)
    case.consts, case.n_temps, case.instrs, case.outs = consts, T, g.instrs, outs
    case.out_degrees = [g.odeg(o) for o in outs]
    case.wire = CS.encode_program(W, NR, consts, T, g.instrs, outs, case.degree)
    return case


def cs_wire_with_degree(case, degree):
    """An instruction-level case's bytes with another declared degree."""
    return CS.encode_program(case.width, case.n_randoms, case.consts, case.n_temps, case.instrs,
                             case.outs, degree)


def code_features(instrs, outs, n_temps):
    """What a program's code contains, by a walk of the tuples: the (op,
    operand kind, position) triples, dst == a / b / both, a temp written again
    with a value of another formal degree, a write nobody reads (dead), a temp
    that holds an untainted, then a tainted, then an untainted value, INV
    operand kinds, INV with dst == a."""
    f = dict(triples=set(), dst_a=False, dst_b=False, dst_ab=False, redegree=False, dead=False,
             taint_cycle=False, inv_kinds=set(), inv_dst_a=False, n_inv=0)
    deg, taint, unread = [None] * n_temps, [False] * n_temps, [False] * n_temps
    hist = [""] * n_temps  # per temp: u / t per value written
    od = lambda o: 1 if o[0] == COL else (deg[o[1]] if o[0] == TEMP else 0)
    ot = lambda o: o[0] == TEMP and taint[o[1]]
    for op, dst, a, b in instrs:
        f["triples"].add((op, a[0], "a"))
        unary = op in (NEG, INV)
        if not unary:
            f["triples"].add((op, b[0], "b"))
        ta, tb = a == (TEMP, dst), (not unary) and b == (TEMP, dst)
        f["dst_ab"] |= ta and tb
        f["dst_a"] |= ta and not tb
        f["dst_b"] |= tb and not ta
        for o in ((a,) if unary else (a, b)):
            if o[0] == TEMP:
                unread[o[1]] = False
        if op == INV:
            f["n_inv"] += 1
            f["inv_kinds"].add(a[0])
            f["inv_dst_a"] |= ta
        d = od(a) if unary else (od(a) + od(b) if op == MUL else max(od(a), od(b)))
        t = op == INV or ot(a) or ((not unary) and ot(b))
        f["redegree"] |= deg[dst] is not None and deg[dst] != d
        f["dead"] |= unread[dst]
        deg[dst], taint[dst], unread[dst] = d, t, True
        hist[dst] += "t" if t else "u"
    for o in outs:
        if o[0] == TEMP:
            unread[o[1]] = False
    f["dead"] |= any(unread)
    f["taint_cycle"] = any("ut" in h and "tu" in h[h.index("ut"):] for h in hist)
    return f


# ---- fill programs ---------------------------------------------------------------

class FillCase:
    """A fill program with its reference.  outputs: [(column, f(row, randoms) ->
    int)]; zeros: per INV (column, f) such that f(row, randoms) is the INV's
    operand and is affine in row[column] (column None: the operand ignores
    the row)."""

    consts = instrs = outs = None
    n_temps = 0

    def __init__(self, level, seed, width, n_randoms, outputs, zeros, wire):
        self.level, self.seed, self.width, self.n_randoms = level, seed, width, n_randoms
        self.outputs, self.zeros, self.wire = outputs, zeros, wire
        self.n_inv = len(zeros)

    def fill_row(self, row, randoms):
        out = list(row)
        for c, f in self.outputs:
            out[c] = f(row, randoms)
        return out

    def fill_matrix(self, m, randoms):
        W = self.width
        return [v for i in range(0, len(m), W) for v in self.fill_row(m[i:i + W], randoms)]

    def make_zero(self, row, randoms, v):
        """Change row so that INV v's operand is zero; False if it cannot be."""
        c, f = self.zeros[v]
        if c is None:
            return f(row, randoms) == 0
        row[c] = 0
        v0 = f(row, randoms)
        row[c] = 1
        slope = (f(row, randoms) - v0) % M
        if slope == 0:
            return False
        row[c] = -v0 * pow(slope, M - 2, M) % M
        assert f(row, randoms) == 0
        return True

    def matrix(self, log_height, threads, K):
        """The matrix for a launch of `threads` lanes with K rows each: zero INV
        operands at the first and at the last of a lane's K rows, at all K rows
        of one lane, and in the last row of the table."""
        h, W = 1 << log_height, self.width
        m = matrix("fill %d %s" % (self.seed, self.level), h, W)
        rnd = self.randoms()
        done = set()
        for i, v in self.zero_rows(log_height, threads, K):
            if i not in done:  # (one zero operand per row: a second would move the first)
                row = m[i * W:(i + 1) * W]
                if self.make_zero(row, rnd, v % self.n_inv):
                    m[i * W:(i + 1) * W] = row
                    done.add(i)
        return m

    def zero_rows(self, log_height, threads, K):
        """(row, which INV) of matrix()'s zero operands, in the table's last chunk
        and in its first; no row twice."""
        if not self.n_inv:
            return []
        h, B = 1 << log_height, threads
        base = (h - 1) // (B * K) * B * K
        rows = [(h - 1, 4), (base + 3 % B, 0), (base + (K - 1) * B + 5 % B, 1)]
        rows += [(base + k * B + 7 % B, 2 + k) for k in range(K)]
        rows += [(k * B + B - 1, 3) for k in (0, K - 1)]  # chunk 0, the last lane
        seen, out = set(), []
        for i, v in rows:
            if i < h and i not in seen:
                seen.add(i)
                out.append((i, v))
        return out

    def randoms(self):
        return elements("fill randoms %d %s" % (self.seed, self.level), self.n_randoms)


def _coefficient(r, width, n_randoms):
    k = r.randrange(3)
    if k == 0:
        j = r.randrange(width)
        return CS.var(j), (lambda x, rn, j=j: x[j])
    if k == 1 and n_randoms:
        j = r.randrange(n_randoms)
        return CS.rand(j), (lambda x, rn, j=j: rn[j])
    c = r.randrange(1, M)
    return CS.const(c), (lambda x, rn, c=c: c)


def fill_expr_case(seed, width=None, n_randoms=None, n_inv=None):
    """{column: Expr} with CS.inv through compile_fill."""
    r = random.Random("fill expr %d" % seed)
    W = _pick(r, width, 1, 32)
    NR = _pick(r, n_randoms, 0 if W > 1 else 1, 4)
    n_inv = n_inv if n_inv is not None else r.choice([0, 1, 2, 5, 16])
    n_out = r.randint(1, min(W, 6))
    cols = sorted(r.sample(range(W), n_out))
    zeros, terms = [], []
    for v in range(n_inv):  # 1 / (base +- var(zc)), base free of zc: never nested
        zc = r.randrange(W)
        g = _ExprGen(r, W, NR, r.randint(0, 3), no_col=zc)
        e, f, _ = g.tree(3)
        if r.random() < 0.5:
            e, f = e + CS.var(zc), (lambda x, rn, f=f, zc=zc: (f(x, rn) + x[zc]) % M)
        else:
            e, f = CS.var(zc) - e, (lambda x, rn, f=f, zc=zc: (x[zc] - f(x, rn)) % M)
        zeros.append((zc, f))
        terms.append((CS.inv(e), (lambda x, rn, f=f: pow(f(x, rn), M - 2, M))))
    per = [[] for _ in cols]  # every inverse goes to one output, in order
    for v in range(n_inv):
        per[v * n_out // n_inv].append(v)
    assign, outputs = {}, []
    for c, vs in zip(cols, per):
        g = _ExprGen(r, W, NR, r.randint(0, 3))
        e, f, _ = g.tree(3)
        if not vs and r.random() < 0.3:
            e, f, _ = g.leaf(1)  # a bare operand as the output
        for v in vs:
            a, fa = _coefficient(r, W, NR)  # not identically zero: the inverse is live
            ie, fi = terms[v]
            e, f = e + a * ie, (lambda x, rn, f=f, fa=fa, fi=fi: (f(x, rn) + fa(x, rn) * fi(x, rn)) % M)
        assign[c] = e
        outputs.append((c, f))
    case = FillCase("expr", seed, W, NR, outputs, zeros, CS.compile_fill(assign, W, NR))
    return case


def fill_instr_case(seed, width=None, n_randoms=None, n_consts=None, n_temps=None, n_inv=None,
                    n_outputs=None, const_zero=False):
    """A fill program in raw instructions (fill_reference.wire's format): INV
    operands of every kind, INV with dst == a, temps reused across taint.
    const_zero: the first INV's operand is the constant zero."""
    import fill_reference as FR

    r = random.Random("fill instr %d" % seed)
    W = _pick(r, width, 1, 32)
    NR, NC = _pick(r, n_randoms, 1, 4), _pick(r, n_consts, 1, 4)
    T = _pick(r, n_temps, 2, 10)
    n_inv = n_inv if n_inv is not None else r.choice([0, 1, 2, 5, 16])
    n_out = _pick(r, n_outputs, 1, min(W, 6))
    g = _CodeGen(r, W, NR, NC, T, 10 ** 9)
    g.reserved = sink = T - 1
    consts = [_const(r) for _ in range(NC)]
    if const_zero:
        consts[0] = 0
    inv_at = []  # (instruction index of the INV, column its operand is affine in or None)
    for _ in range(r.randint(1, 4)):
        g.arith()
    for v in range(n_inv):
        kind = r.choice([COL, RAND, CONST, TEMP, TEMP, TEMP])
        if const_zero and v == 0:
            a, zc = (CONST, 0), None
        elif kind == COL:
            zc = r.randrange(W)
            a = (COL, zc)
        elif kind == RAND:
            a, zc = (RAND, r.randrange(NR)), None
        elif kind == CONST:
            a, zc = (CONST, r.randrange(NC)), None
        else:  # a temp: x +- column zc with x free of zc and of any INV
            zc = r.randrange(W)
            x = g.operand(tainted=False, avoid=zc)
            t = r.randrange(T - 1)
            if r.random() < 0.5:
                g.emit(ADD, t, x, (COL, zc))
            else:
                g.emit(SUB, t, (COL, zc), x)
            a = (TEMP, t)
        # dst == a; or a temp that held an untainted value (so that it goes
        # untainted -> tainted here, and later code may rewrite it untainted)
        dst = a[1] if (a[0] == TEMP and r.random() < 0.4) else r.randrange(T - 1)
        inv_at.append((len(g.instrs), zc))
        g.emit(INV, dst, a)
        # every inverse reaches an output through the sink temp T - 1
        if g.deg[sink] is None:
            g.emit(MUL, sink, (TEMP, dst), (COL, r.randrange(W)))
        else:
            g.emit(r.choice([ADD, SUB]), sink, (TEMP, sink), (TEMP, dst))
        for _ in range(r.randint(0, 3)):
            g.arith()                    # may read and overwrite tainted temps
        if r.random() < 0.5:             # the INV's temp written again, untainted
            g.emit(r.choice([ADD, MUL]), dst, g.operand(tainted=False), g.operand(tainted=False))
    for _ in range(r.randint(0, 4)):
        g.arith()
    cols = sorted(r.sample(range(W), n_out))
    outs = []
    for c in cols:
        o = (TEMP, r.choice(g.written())) if r.random() < 0.75 else g.operand()
        outs.append((c, o[0], o[1]))
    if n_inv:
        k = r.randrange(n_out)
        outs[k] = (outs[k][0], TEMP, sink)
    ref = _Interp(W, NR, consts, T, g.instrs)
    outputs = [(c, (lambda x, rn, o=(k, i): ref.operand(x, rn, o))) for c, k, i in outs]
    zeros = []
    for at, zc in inv_at:
        a = g.instrs[at][2]
        zeros.append((zc, (lambda x, rn, at=at, a=a: ref.run(x, rn, at)[ref.off[a[0]] + a[1]])))
    case = FillCase("instr", seed, W, NR, outputs, zeros, FR.wire(W, NR, consts, T, g.instrs, outs))
    case.consts, case.n_temps, case.instrs, case.outs = consts, T, g.instrs, outs
    case.taint = list(g.taint)
    return case


def fill_case(seed, level="expr", **pins):
    return fill_expr_case(seed, **pins) if level == "expr" else fill_instr_case(seed, **pins)


def fill_wire_with(case, extra):
    """An instruction-level fill case's bytes with `extra` instructions appended."""
    import fill_reference as FR

    return FR.wire(case.width, case.n_randoms, case.consts, case.n_temps, case.instrs + extra,
                   case.outs)


# ---- the committed cases -----------------------------------------------------------
# seed, kind and pins feed the generator; width, log_height and threads are what it
# must give (the CPU test asserts them).  log_height: the top height, at which the
# first pass has two blocks and four row pairs per thread (2^10 / 2^11 / 2^12 for 64
# / 128 / 256 threads); `small`: a limit program, run at this height only.  sums:
# the case runs through mlh_cs_sumcheck_prove_sums with this sum-column mask
# ("bit0", "top", "all" or "random").


def _cs(seed, kind, width, log_height, threads, sums=None, small=False, **pins):
    return dict(seed=seed, kind=kind, width=width, log_height=log_height, threads=threads,
                sums=sums, small=small, pins=dict(pins, width=width))


CS_TABLE = [
    _cs(1, "expr", 1, 12, 256, degree=1, n_constraints=1),
    _cs(2, "expr", 3, 12, 256, sums="bit0", degree=2),
    _cs(3, "expr", 5, 12, 256, degree=3, n_constraints=5),
    _cs(4, "expr", 7, 12, 256, sums="top", degree=4),
    _cs(5, "expr", 6, 12, 256, degree=5),
    _cs(6, "expr", 4, 12, 256, degree=6),
    _cs(7, "expr", 9, 12, 256, sums="random", degree=7),
    _cs(8, "expr", 17, 11, 128, degree=4),
    _cs(9, "expr", 19, 11, 128, sums="all", degree=6, n_constraints=7),
    _cs(10, "expr", 24, 11, 128, degree=7),
    _cs(31, "expr", 32, 11, 128, sums="top", degree=2, n_constraints=3),
    _cs(12, "expr", 32, 10, 64, degree=7, n_constraints=12),   # 13 temps: 85 slots
    _cs(13, "expr", 13, 12, 256, degree=3),
    _cs(14, "expr", 2, 12, 256, sums="all", degree=5),
    _cs(15, "expr", 18, 11, 128, degree=1),
    _cs(16, "expr", 30, 10, 64, sums="random", degree=5, n_constraints=11),  # 13 temps: 79 slots
    _cs(37, "expr", 11, 12, 256, degree=2, n_constraints=3),
    _cs(18, "expr", 8, 12, 256, degree=4, n_constraints=6),
    _cs(1, "instr", 7, 12, 256),
    _cs(2, "instr", 32, 10, 64, sums="random", n_temps=32, degree=7, n_instr=250),  # 104 slots
    _cs(3, "instr", 25, 10, 64, n_temps=20, degree=6),          # 77 slots: the first at 64 threads
    _cs(4, "instr", 32, 11, 128, sums="bit0", n_temps=8, degree=3),  # 76 slots: the last at 128
    _cs(5, "instr", 12, 11, 128, n_temps=12, degree=4),
    _cs(6, "instr", 5, 12, 256, sums="all", n_randoms=64, n_consts=64, n_constraints=37,
        n_instr=300, degree=3),                                 # mask indices 128..164
    _cs(7, "instr", 3, 5, 256, small=True, n_constraints=256, degree=2),
    _cs(8, "instr", 4, 6, 256, small=True, n_instr=4096, n_temps=6, degree=3),
    _cs(9, "instr", 1, 12, 256, n_temps=3),
    _cs(10, "instr", 21, 10, 64, degree=7, n_temps=27),
    _cs(11, "instr", 10, 12, 256, sums="top", degree=1),
    _cs(12, "instr", 15, 11, 128, n_temps=5, degree=5),
]


# log_height, threads: one chunk of the default shape (one row per thread at these
# heights).  shapes: (threads, rows per thread, log_height) of the two explicit
# launches of a program with an INV: 16 rows per thread below threads x 16 rows,
# so that some lanes have no row, and two chunks of another shape.
def _fill(seed, kind, width, n_inv, log_height, threads, shapes, **pins):
    return dict(seed=seed, kind=kind, width=width, n_inv=n_inv, log_height=log_height,
                threads=threads, shapes=shapes, pins=dict(pins, width=width, n_inv=n_inv))


FILL_TABLE = [
    _fill(1, "expr", 1, 0, 8, 256, []),
    _fill(2, "expr", 2, 1, 8, 256, [(64, 16, 8), (256, 2, 10)]),
    _fill(3, "expr", 3, 2, 8, 256, [(128, 16, 10), (128, 4, 10)]),
    _fill(4, "expr", 5, 5, 8, 256, [(256, 16, 10), (256, 8, 12)]),
    _fill(5, "expr", 7, 16, 8, 256, [(64, 16, 8), (64, 2, 8)]),
    _fill(6, "expr", 12, 0, 8, 256, []),
    _fill(7, "expr", 17, 2, 8, 256, [(128, 16, 9), (256, 4, 11)]),
    _fill(8, "expr", 32, 5, 7, 128, [(64, 16, 9), (64, 4, 9)]),
    _fill(9, "expr", 32, 16, 7, 128, [(64, 16, 9), (64, 4, 9)]),
    _fill(10, "expr", 9, 1, 8, 256, [(64, 16, 9), (64, 4, 9)]),
    _fill(11, "expr", 26, 1, 8, 256, [(64, 16, 8), (128, 2, 9)]),
    _fill(12, "expr", 4, 2, 8, 256, [(128, 16, 10), (256, 4, 11)]),
    _fill(1, "instr", 3, 2, 8, 256, [(64, 16, 8), (64, 4, 9)]),
    _fill(2, "instr", 32, 16, 6, 64, [(64, 16, 8), (64, 2, 8)], n_temps=32),   # 80 slots
    _fill(3, "instr", 32, 16, 6, 64, [(64, 16, 9), (64, 4, 9)], n_temps=32, n_outputs=32),
    _fill(4, "instr", 20, 16, 7, 128, [(64, 16, 8), (64, 4, 9)], n_temps=10),
    _fill(5, "instr", 5, 5, 8, 256, [(64, 16, 8), (64, 4, 9)], const_zero=True),
    _fill(6, "instr", 1, 1, 8, 256, [(128, 16, 9), (256, 2, 10)]),
    _fill(7, "instr", 6, 0, 8, 256, []),
    _fill(8, "instr", 13, 5, 8, 256, [(128, 16, 10), (128, 4, 10)]),
    _fill(9, "instr", 32, 2, 7, 128, [(128, 16, 9), (64, 8, 10)], n_temps=12),
    _fill(10, "instr", 7, 16, 8, 256, [(64, 16, 9), (64, 4, 9)], n_temps=8),
    _fill(11, "instr", 11, 1, 8, 256, [(128, 16, 9), (64, 8, 10)]),
    _fill(12, "instr", 2, 5, 8, 256, [(128, 16, 10), (64, 4, 9)]),
]


def cs_case(entry):
    pins = dict(entry.get("pins", {}))
    case = (expr_case if entry["kind"] == "expr" else instr_case)(entry["seed"], **pins)
    case.name = "%s%d" % (entry["kind"], entry["seed"])
    case.log_height = entry["log_height"]
    return case


def sum_mask(entry, width):
    kind = entry.get("sums")
    if not kind:
        return 0
    if kind == "bit0":
        return 1
    if kind == "top":
        return 1 << (width - 1)
    if kind == "all":
        return (1 << width) - 1
    r = random.Random("sums %d" % entry["seed"])
    return r.randrange(1, 1 << width)


def fill_table_case(entry):
    case = fill_case(entry["seed"], entry["kind"], **dict(entry.get("pins", {})))
    case.name = "fill_%s%d" % (entry["kind"], entry["seed"])
    return case
