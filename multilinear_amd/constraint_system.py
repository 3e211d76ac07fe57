"""Constraint system (src/constraint_system) on the MI355X: System /
ChallengeSet / ConstraintSet / Trace and the general sumcheck prover and
verifier of constraint_system/sumcheck.rs:21-125,147-256.

The reference's ``Expr<F>(fn(&[F], &[F]) -> F)`` (constraints.rs:3-10) becomes
a constraint program: expressions built here from ``var(j)``, ``rand(k)``,
integers and ``+ - *`` compile to the straight-line wire format of
include/mlhip.h, which libmlhip validates, interprets on the device (prover)
and on the host (verifier).  ``Commitment`` is a TODO in the reference
(trace.rs:41-48); here it is the commit phase of the batched PCS over the
trace's columns (mlh_trace_commit), and ``System.committed_prover`` /
``System.prove`` / ``SystemProof.verify`` compose it with the sumcheck into a
proof a verifier checks without the trace (mlh_system_prove / _verify).
``WitnessLayout.pre_random_columns`` and ``sum_columns`` (system.rs:23-29) are
the two-phase proof: ``System.phased_prover`` commits to the pre-random
columns and hands out the trace randoms, the caller fills the other columns
(``PhasedProver.fill`` / ``Trace.fill``: a fill program, expressions with
``inv``, run in place by mlh_trace_fill; or ``field_inv`` and the other field
ops below on column vectors), and ``prove`` / ``PhasedSystemProof.verify`` are
mlh_system_prove_phased / _verify_phased, the column sum by default from
mlh_trace_column_sum.  A constraint set may refer to the next row with
``nxt(j)`` (a shifted system: ``compile_shifted``, ``Trace.extend_next``);
``PhasedProver.prove`` then runs mlh_system_prove_shifted and returns a
``ShiftedSystemProof``.  The last columns of a layout may be public
(``WitnessLayout(public_columns=PublicColumns()...)``: selectors, constants,
the row index, periodic tables, sparse public inputs): ``phased_prover`` writes
them with ``Trace.fill_public`` (mlh_trace_fill_public), commits only the
columns below them and proves with mlh_system_prove_public, and
``ShiftedSystemProof.verify`` evaluates the spec itself
(mlh_system_verify_public).  A lookup's multiplicity column, which is pre-random, is
counted in place before ``phased_prover`` by ``Trace.lookup_multiplicities``
(mlh_trace_lookup_counts), or, for keys of several columns such as (x, y, x ^ y),
by ``Trace.lookup_tuple_multiplicities`` (mlh_trace_lookup_tuple_counts);
``tuple_key`` spells the compressed key of such a lookup for the fill and the
constraint.  The column a next-row constraint ``nxt(z) - z * t`` or ``nxt(z) -
z - t`` holds (a grand product, a running sum) is written in phase 2 by
``PhasedProver.scan`` / ``Trace.scan`` (mlh_trace_scan), which also return the
total across the cyclic wrap.  A sorted copy of columns (a memory log in
address-then-timestamp order, the ordered side of a multiset argument) is
written by ``PhasedProver.sort`` / ``Trace.sort`` (mlh_trace_sort).  Before
``prove``, ``PhasedProver.check`` / ``Trace.check`` / ``Trace.check_public``
(mlh_trace_check, mlh_trace_check_public) say which constraint fails on how many rows and where first, and whether the
public strip is the spec's.
"""
import ctypes
import struct

from . import _lib
from .batched import BatchedPCSProof
from .device import M, check, context, empty, fe_bytes, fe_from_bytes, lib, ptr
from .polynomials import eq_table
from .transcript import Transcript

OP_ADD, OP_SUB, OP_MUL, OP_NEG, OP_INV = 0, 1, 2, 3, 4
COL, RAND, CONST, TEMP = 0, 1, 2, 3
MAX_TEMPS = 32
MAX_INVERSES = 16


# ---- expressions -------------------------------------------------------------

class Expr:
    """A node of a constraint expression (leaf: column / random / constant)."""

    __slots__ = ("op", "args")

    def __init__(self, op, *args):
        self.op = op
        self.args = args

    @staticmethod
    def wrap(v):
        if isinstance(v, Expr):
            return v
        if isinstance(v, int):
            return Expr("const", v % M)  # the integer's residue mod M
        raise TypeError("constraint expressions take Expr or int operands, not %r" % type(v))

    def __add__(self, o):
        return Expr("add", self, Expr.wrap(o))

    def __radd__(self, o):
        return Expr("add", Expr.wrap(o), self)

    def __sub__(self, o):
        return Expr("sub", self, Expr.wrap(o))

    def __rsub__(self, o):
        return Expr("sub", Expr.wrap(o), self)

    def __mul__(self, o):
        return Expr("mul", self, Expr.wrap(o))

    def __rmul__(self, o):
        return Expr("mul", Expr.wrap(o), self)

    def __neg__(self):
        return Expr("neg", self)


def var(j):
    """Column j of the row (the closure's ``var[j]``)."""
    return Expr("var", int(j))


def rand(k):
    """Random challenge k (the closure's second argument)."""
    return Expr("rand", int(k))


def const(v):
    return Expr.wrap(int(v))


def inv(e):
    """1 / e, zero -> zero (field.rs:113-118); fill programs only."""
    return Expr("inv", Expr.wrap(e))


def nxt(j):
    """Column j of the next row, (i + 1) mod height at row i: a shifted column
    of a shifted system (compile_shifted; include/mlhip.h)."""
    return Expr("nxt", int(j))


# ---- wire format -------------------------------------------------------------

def encode_program(width, n_randoms, consts, n_temps, instrs, outs, degree):
    """The wire format of include/mlhip.h.  instrs: (op, dst, (kind, index),
    (kind, index)) -- NEG takes (0, 0) as its second operand; outs: (kind,
    index) per constraint."""
    b = struct.pack("<7I", width, n_randoms, len(consts), n_temps, len(instrs), len(outs), degree)
    b += b"".join(int(c).to_bytes(16, "little") for c in consts)
    for op, dst, a, bb in instrs:
        b += bytes([op, dst, a[0], a[1], bb[0], bb[1], 0, 0])
    for o in outs:
        b += bytes([o[0], o[1]])
    return b


_OPS = {"add": OP_ADD, "sub": OP_SUB, "mul": OP_MUL}
_UNARY = {"neg": OP_NEG, "inv": OP_INV}


def _emit_outputs(exprs, allow_inv):
    """Expressions -> (consts, n_temps, instrs, output operands): what
    compile_program and compile_fill share.  Straight-line code in evaluation
    order; a temp is released when its value has been consumed, the deeper
    operand of a binary node is evaluated first, and equal constants share a
    pool entry."""
    consts, instrs, free, live, n_inv = [], [], [], [0], [0]
    need_memo, inv_memo = {}, {}

    def need(e):  # temps needed to evaluate e (Sethi-Ullman)
        k = id(e)
        if k not in need_memo:
            if e.op in ("var", "rand", "const", "nxt"):
                need_memo[k] = 0
            elif e.op in _UNARY:
                need_memo[k] = max(1, need(e.args[0]))
            else:
                a, b = need(e.args[0]), need(e.args[1])
                need_memo[k] = max(1, a + 1 if a == b else max(a, b))
        return need_memo[k]

    def has_inv(e):
        k = id(e)
        if k not in inv_memo:
            inv_memo[k] = e.op == "inv" or (e.op not in ("var", "rand", "const")
                                            and any(has_inv(a) for a in e.args))
        return inv_memo[k]

    def alloc():
        if free:
            return free.pop()
        t = live[0]
        if t >= MAX_TEMPS:
            raise ValueError("constraint program needs more than %d temps" % MAX_TEMPS)
        live[0] += 1
        return t

    def release(o):
        if o[0] == TEMP:
            free.append(o[1])

    def emit(e):
        if e.op == "var":
            return (COL, e.args[0])
        if e.op == "rand":
            return (RAND, e.args[0])
        if e.op == "nxt":
            raise ValueError("nxt() needs a shifted system (compile_shifted)")
        if e.op == "const":
            if e.args[0] not in consts:
                consts.append(e.args[0])
            return (CONST, consts.index(e.args[0]))
        if e.op in _UNARY:
            if e.op == "inv":
                if not allow_inv:
                    raise ValueError("a constraint program has no inverse (fill programs do)")
                if has_inv(e.args[0]):
                    raise ValueError("nested inverse: an inv() operand may not contain an inv()")
                n_inv[0] += 1
                if n_inv[0] > MAX_INVERSES:
                    raise ValueError("fill program needs more than %d inverses" % MAX_INVERSES)
            a = emit(e.args[0])
            release(a)
            dst = alloc()
            instrs.append((_UNARY[e.op], dst, a, (0, 0)))
            return (TEMP, dst)
        if need(e.args[1]) > need(e.args[0]):
            b = emit(e.args[1])
            a = emit(e.args[0])
        else:
            a = emit(e.args[0])
            b = emit(e.args[1])
        release(a)
        release(b)
        dst = alloc()
        instrs.append((_OPS[e.op], dst, a, b))
        return (TEMP, dst)

    outs = [emit(Expr.wrap(e)) for e in exprs]  # (an output's temp is never released)
    return consts, live[0], instrs, outs


def compile_program(exprs, width, n_randoms, degree):
    """Expressions -> wire bytes of a constraint program (_emit_outputs).
    ValueError for an ``inv`` node."""
    consts, n_temps, instrs, outs = _emit_outputs(exprs, allow_inv=False)
    return encode_program(width, n_randoms, consts, n_temps, instrs, outs, degree)


def compile_shifted(exprs, width, n_randoms, degree):
    """Expressions with ``nxt`` -> (wire bytes, shift list): the distinct
    ``nxt`` columns in order of first appearance become columns width, width +
    1, ... of an ordinary program of width ``width + len(shift list)``, the
    program mlh_system_prove_shifted takes beside the list.  Without ``nxt``
    the bytes are compile_program's and the list is empty."""
    shifts, memo = [], {}

    def rewrite(e):
        k = id(e)
        if k not in memo:
            if e.op == "nxt":
                c = e.args[0]
                if not 0 <= c < width:
                    raise ValueError("nxt(%r): column outside the trace" % (c,))
                if c not in shifts:
                    shifts.append(c)
                memo[k] = var(width + shifts.index(c))
            elif e.op in ("var", "rand", "const"):
                memo[k] = e
            else:
                memo[k] = Expr(e.op, *[rewrite(a) for a in e.args])
        return memo[k]

    exprs = [Expr.wrap(e) for e in exprs]  # (kept alive: the memo is keyed by id)
    out = [rewrite(e) for e in exprs]
    if width + len(shifts) > 32:
        raise ValueError("%d columns and %d shifted ones are more than 32" % (width, len(shifts)))
    return compile_program(out, width + len(shifts), n_randoms, degree), shifts


def compile_fill(assignments, width, n_randoms):
    """{column: Expr} -> wire bytes of a fill program (include/mlhip.h): the
    code of compile_program with ``inv``, outputs in ascending column order.
    ValueError for a nested inverse or more than 16 of them."""
    cols = sorted(assignments)
    for c in cols:
        if not 0 <= c < width:
            raise ValueError("output column %r outside the trace" % (c,))
    consts, n_temps, instrs, outs = _emit_outputs([assignments[c] for c in cols], allow_inv=True)
    b = struct.pack("<7I", width, n_randoms, len(consts), n_temps, len(instrs), len(outs), 0)
    b += b"".join(int(c).to_bytes(16, "little") for c in consts)
    for op, dst, a, bb in instrs:
        b += bytes([op, dst, a[0], a[1], bb[0], bb[1], 0, 0])
    for c, o in zip(cols, outs):
        b += bytes([c, o[0], o[1], 0])
    return b


class FillProgram:
    """A validated fill program (mlh_fill_program)."""

    def __init__(self, wire):
        self.wire = bytes(wire)
        h = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * len(self.wire)).from_buffer_copy(self.wire)
        check(lib().mlh_fill_program_create(buf, len(self.wire), ctypes.byref(h)))
        self.h = h.value
        self.width = lib().mlh_fill_program_width(self.h)
        self.n_randoms = lib().mlh_fill_program_n_randoms(self.h)
        self.n_outputs = lib().mlh_fill_program_n_outputs(self.h)
        self.n_inverses = lib().mlh_fill_program_n_inverses(self.h)
        self.output_mask = lib().mlh_fill_program_output_mask(self.h)

    def __del__(self):
        try:
            lib().mlh_fill_program_destroy(self.h)
        except Exception:
            pass

    def evaluate(self, row, randoms):
        """The row after the fill, by the host interpreter."""
        out = (ctypes.c_uint8 * (16 * self.width))()
        check(lib().mlh_fill_program_evaluate(self.h, _elems(row), _elems(randoms), out))
        return _split(out, self.width)

    def launch_info(self, log_height):
        """(threads per block, rows per thread and inversion, blocks)."""
        t, k, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().mlh_trace_fill_launch_info(self.h, log_height, ctypes.byref(t), ctypes.byref(k),
                                               ctypes.byref(b)))
        return t.value, k.value, b.value


class Program:
    """A validated constraint program (mlh_cs_program)."""

    def __init__(self, wire):
        self.wire = bytes(wire)
        h = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * len(self.wire)).from_buffer_copy(self.wire)
        check(lib().mlh_cs_program_create(buf, len(self.wire), ctypes.byref(h)))
        self.h = h.value
        self.width = lib().mlh_cs_program_width(self.h)
        self.degree = lib().mlh_cs_program_degree(self.h)
        self.n_constraints = lib().mlh_cs_program_n_constraints(self.h)
        self.n_randoms = lib().mlh_cs_program_n_randoms(self.h)

    def __del__(self):
        try:
            lib().mlh_cs_program_destroy(self.h)
        except Exception:
            pass

    def evaluate(self, values, randoms, mask):
        """ConstraintSet::evaluate (evaluation.rs:21-29) by the host interpreter."""
        out = (ctypes.c_uint8 * 16)()
        check(lib().mlh_cs_program_evaluate(self.h, _elems(values), _elems(randoms), _elems(mask),
                                            out))
        return fe_from_bytes(out)

    def launch_info(self, log_height):
        """(threads per block, blocks) of the first pass over 2^log_height rows."""
        t, b = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().mlh_cs_launch_info(self.h, log_height, ctypes.byref(t), ctypes.byref(b)))
        return t.value, b.value


PC_CONST, PC_FIRST, PC_LAST, PC_ROW, PC_PERIODIC, PC_SPARSE = 0, 1, 2, 3, 4, 5


def _le16(v):
    return (int(v) % M).to_bytes(16, "little")


class PublicColumns:
    """The public columns of a trace, its last ``len(self)`` ones: columns with
    a short description that the prover neither commits nor opens and the
    verifier evaluates itself (mlh_public_columns, include/mlhip.h).  A builder:
    each call appends one column and returns the builder.  ``wire`` is the
    encoded spec; the handle behind ``h`` is made from it on first use and
    needs no GPU."""

    def __init__(self):
        self._cols = []  # (kind, arg, payload bytes)
        self._handle = None

    def _add(self, kind, arg, payload=b""):
        if self._handle is not None:
            raise ValueError("the spec is in use: build a new one")
        self._cols.append((kind, arg, payload))
        return self

    def const(self, c):
        """Every row holds c."""
        return self._add(PC_CONST, 0, _le16(c))

    def first(self):
        """1 at row 0, else 0."""
        return self._add(PC_FIRST, 0)

    def last(self):
        """1 at the last row, else 0."""
        return self._add(PC_LAST, 0)

    def row_index(self):
        """Row i holds i."""
        return self._add(PC_ROW, 0)

    def periodic(self, values):
        """Row i holds values[i mod len(values)]; the length is a power of two."""
        values = list(values)
        n = len(values)
        if n < 1 or n & (n - 1):
            raise ValueError("a periodic column takes a power-of-two number of values")
        return self._add(PC_PERIODIC, n.bit_length() - 1, b"".join(_le16(v) for v in values))

    def sparse(self, entries):
        """{row: value}; zero on every other row."""
        items = sorted((int(r), v) for r, v in dict(entries).items())
        return self._add(PC_SPARSE, len(items),
                         b"".join(struct.pack("<Q", r) + _le16(v) for r, v in items))

    def __len__(self):
        return len(self._cols)

    @property
    def wire(self):
        return struct.pack("<2I", len(self._cols), 0) + b"".join(
            struct.pack("<2I", kind, arg) + payload for kind, arg, payload in self._cols)

    @property
    def h(self):
        if self._handle is None:
            w = self.wire
            h = ctypes.c_void_p()
            buf = (ctypes.c_uint8 * len(w)).from_buffer_copy(w)
            check(lib().mlh_public_columns_create(buf, len(w), ctypes.byref(h)))
            self._handle = h.value
        return self._handle

    def __del__(self):
        try:
            if self._handle is not None:
                lib().mlh_public_columns_destroy(self._handle)
        except Exception:
            pass

    @property
    def digest(self):
        out = (ctypes.c_uint8 * 32)()
        check(lib().mlh_public_columns_digest(self.h, out))
        return bytes(out)

    def evaluate(self, point):
        """The columns' multilinear extensions over 2^len(point) rows at
        ``point``, on the host (mlh_public_columns_evaluate)."""
        point = list(point)
        out = (ctypes.c_uint8 * (16 * len(self)))()
        check(lib().mlh_public_columns_evaluate(self.h, len(point), _elems(point), out))
        return _split(out, len(self))


def public_fill_launch_info(log_height, width, n_public):
    """(rows per tile, blocks) of mlh_trace_fill_public."""
    rows, blocks = ctypes.c_uint32(), ctypes.c_uint32()
    check(lib().mlh_trace_fill_public_launch_info(log_height, width, n_public, ctypes.byref(rows),
                                                  ctypes.byref(blocks)))
    return rows.value, blocks.value


def _elems(vals):
    vals = list(vals)
    if not vals:
        return None
    return (ctypes.c_uint8 * (16 * len(vals))).from_buffer_copy(
        b"".join(int(v).to_bytes(16, "little") for v in vals))


def _split(raw, n):
    raw = bytes(raw)
    return [fe_from_bytes(raw[16 * i:16 * i + 16]) for i in range(n)]


# ---- the reference's types ---------------------------------------------------

class ConstraintSet:
    """constraints.rs:12-34: constraints ``expr = 0`` and their degree."""

    def __init__(self, constraints, degree):
        self._constraints = [Expr.wrap(e) for e in constraints]
        self._degree = degree

    def constraints(self):
        return self._constraints

    def degree(self):
        return self._degree


class WitnessLayout:
    """system.rs:17-30.  public_columns (a PublicColumns; None: none): the last
    len(public_columns) of ``columns`` are public -- not committed, derived by
    the verifier."""

    def __init__(self, columns, randoms=0, pre_random_columns=0, sum_columns=(),
                 public_columns=None):
        self.columns = columns
        self.randoms = randoms
        self.pre_random_columns = pre_random_columns
        self.sum_columns = tuple(sum_columns)
        if public_columns is not None and not len(public_columns):
            public_columns = None  # an empty builder: no public columns
        self.public_columns = public_columns

    @property
    def n_public(self):
        return len(self.public_columns) if self.public_columns is not None else 0


class Trace:
    """trace.rs:5-39: a row-major height x width matrix on the device
    ((height * width, 4) int32 limbs)."""

    def __init__(self, dev_matrix, width):
        n = dev_matrix.shape[0]
        assert width >= 1 and n % width == 0
        self._matrix = dev_matrix
        self._width = width
        self._height = n // width
        assert self._height & (self._height - 1) == 0 and self._height > 0

    def matrix(self):
        return self._matrix

    def width(self):
        return self._width

    def height(self):
        return self._height

    def evaluate(self, points, device=0):
        """evaluation.rs:31-48 (mlh_trace_evaluate)."""
        ctx = context(device)
        out = (ctypes.c_uint8 * (16 * self._width))()
        check(lib().mlh_trace_evaluate(ctx, ptr(self._matrix), self._height.bit_length() - 1,
                                       self._width, _elems(points), out), ctx)
        return _split(out, self._width)

    def fill(self, program_or_assignments, randoms, device=0):
        """Run a fill program on every row, in place (mlh_trace_fill): a
        FillProgram, or {column: Expr} compiled for this width and randoms."""
        prog = program_or_assignments
        if not isinstance(prog, FillProgram):
            prog = FillProgram(compile_fill(prog, self._width, len(randoms)))
        if len(randoms) != prog.n_randoms:
            raise ValueError("the fill program takes %d randoms" % prog.n_randoms)
        ctx = context(device)
        check(lib().mlh_trace_fill(ctx, prog.h, ptr(self._matrix), self._height.bit_length() - 1,
                                   self._width, _elems(randoms)), ctx)
        return prog

    def fill_public(self, spec, device=0):
        """Write the public columns ``spec`` (a PublicColumns) into the last
        len(spec) columns of every row, in place (mlh_trace_fill_public)."""
        ctx = context(device)
        check(lib().mlh_trace_fill_public(ctx, spec.h, ptr(self._matrix),
                                          self._height.bit_length() - 1, self._width), ctx)
        return spec

    def scan(self, scans, device=0, totals=True):
        """Running sums and running products down columns, in place
        (mlh_trace_scan).  ``scans``: a list of (op, src, dst, init), op "add"
        or "mul": column dst becomes z with z[0] = init and z[i + 1] = z[i] op
        t[i], t the column src as it stood at the call.  Returns the list of
        totals z[height - 1] op t[height - 1], or None when ``totals`` is false
        (the call then does not wait for the device)."""
        ops, src, dst, inits = _scan_arrays(scans, self._width)
        n = len(ops)
        out = (ctypes.c_uint8 * (16 * n))() if totals else None
        ctx = context(device)
        check(lib().mlh_trace_scan(ctx, ptr(self._matrix), self._height.bit_length() - 1,
                                   self._width, n, (ctypes.c_uint8 * n)(*ops),
                                   (ctypes.c_uint8 * n)(*src), (ctypes.c_uint8 * n)(*dst),
                                   _elems(inits), out), ctx)
        return _split(out, n) if totals else None

    def sort(self, keys, copies, perm_column=None, device=0, shape=None):
        """Sorted copies of columns, in place (mlh_trace_sort).  ``keys``: 1 to
        4 key columns, the most significant first, compared as unsigned 128-bit
        integers; ``copies``: up to 16 (src, dst) pairs: column dst becomes
        column src in stable ascending key order; ``perm_column`` (or None)
        receives the source row of every sorted row.  ``shape``: None for the
        default launch, or (threads, rows_per_thread, max_blocks[, flags]) for
        mlh_trace_sort_shaped.  Returns the number of digit passes that ran."""
        key, src, dst, perm = _sort_arrays(keys, copies, perm_column, self._width)
        u32s = lambda v: (ctypes.c_uint32 * max(len(v), 1))(*v)
        passes = ctypes.c_uint32()
        ctx = context(device)
        args = (ctx, ptr(self._matrix), self._height.bit_length() - 1, self._width, len(key),
                u32s(key), len(src), u32s(src), u32s(dst), perm, ctypes.byref(passes))
        if shape is None:
            check(lib().mlh_trace_sort(*args), ctx)
        else:
            threads, rows, max_blocks = shape[:3]
            flags = shape[3] if len(shape) > 3 else 0
            check(lib().mlh_trace_sort_shaped(*args, threads, rows, max_blocks, flags), ctx)
        return passes.value

    def extend_next(self, shift_columns, device=0):
        """The extension of a shifted system (mlh_trace_extend_next): a new
        Trace of width + len(shift_columns) columns whose column width + k is
        column shift_columns[k] of the next row, cyclically; this trace is not
        modified."""
        cols = [int(c) for c in shift_columns]
        K, L = len(cols), self._height.bit_length() - 1
        ctx = context(device)
        out = empty(self._height * (self._width + K), device)
        arr = (ctypes.c_uint32 * max(K, 1))(*cols)
        check(lib().mlh_trace_extend_next(ctx, ptr(self._matrix), L, self._width, arr, K, ptr(out)),
              ctx)
        return Trace(out, self._width + K)

    def check(self, program, randoms=(), shift_columns=(), device=0, shape=None):
        """Run every constraint of ``program`` (a Program of width + len(
        shift_columns) columns, as compile_shifted gives it beside the list) on
        every row, the shifted columns read from the next row, cyclically
        (mlh_trace_check).  Returns a CheckResult; the trace is not modified.
        shape = (threads, max_blocks): mlh_trace_check_shaped."""
        cols, randoms = _check_arguments(self._width, program, randoms, shift_columns)
        K, n = len(cols), program.n_constraints
        counts, firsts = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
        rep = _lib.TraceCheckReportC()
        args = (program.h, ptr(self._matrix), self._height.bit_length() - 1, self._width,
                (ctypes.c_uint32 * max(K, 1))(*cols), K, _elems(randoms), counts, firsts,
                ctypes.byref(rep))
        ctx = context(device)
        if shape is None:
            check(lib().mlh_trace_check(ctx, *args), ctx)
        else:
            check(lib().mlh_trace_check_shaped(ctx, *args, *shape), ctx)
        return CheckResult(rep.n_bad_rows, rep.first_bad_row, rep.first_bad_constraint,
                           list(counts), list(firsts))

    def check_public(self, spec, device=0):
        """The last len(spec) columns against what ``fill_public(spec)`` would
        write (mlh_trace_check_public).  Returns a CheckResult per public
        column; ``first_bad_constraint`` is the lowest column of the strip that
        differs on the first bad row.  The trace is not modified."""
        n = len(spec)
        counts, firsts = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
        bad, first = ctypes.c_uint64(), ctypes.c_uint64()
        ctx = context(device)
        check(lib().mlh_trace_check_public(ctx, spec.h, ptr(self._matrix),
                                           self._height.bit_length() - 1, self._width, counts,
                                           firsts, ctypes.byref(bad), ctypes.byref(first)), ctx)
        firsts = list(firsts)
        col = firsts.index(first.value) if bad.value else _NONE32
        return CheckResult(bad.value, first.value, col, list(counts), firsts)

    def lookup_counts(self, value_columns, table_column, count_column, device=0):
        """A lookup's multiplicities, in place (mlh_trace_lookup_counts): column
        ``count_column`` of the lowest row holding each entry of ``table_column``
        receives how often that entry occurs in ``value_columns``, the other
        rows zero.  Returns (n_missing, first_missing_row): the (row, value
        column) pairs whose value is no table entry and the lowest such row,
        None when nothing is missing."""
        mask = _lookup_mask(self._width, value_columns, table_column, count_column)
        ctx = context(device)
        n, first = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().mlh_trace_lookup_counts(ctx, ptr(self._matrix), self._height.bit_length() - 1,
                                            self._width, mask, table_column, count_column,
                                            ctypes.byref(n), ctypes.byref(first)), ctx)
        return n.value, (None if first.value == 2 ** 64 - 1 else first.value)

    def lookup_multiplicities(self, value_columns, table_column, count_column, device=0):
        """lookup_counts for a lookup that must hold: ValueError naming the
        first row with a value that is no table entry."""
        n, first = self.lookup_counts(value_columns, table_column, count_column, device)
        if n:
            raise ValueError("%d looked-up value%s not in table column %d, the first in row %d"
                             % (n, "" if n == 1 else "s", table_column, first))

    def lookup_tuple_counts(self, value_tuples, table_columns, count_column, selectors=None,
                            device=0):
        """A tuple lookup's multiplicities, in place
        (mlh_trace_lookup_tuple_counts): the key of a row is its
        ``table_columns`` in that order, and column ``count_column`` of the
        lowest row holding each key receives how many enabled (row, tuple)
        pairs of ``value_tuples`` (each a column list as long as
        ``table_columns``) hold it, the other rows zero.  ``selectors``: None,
        or per tuple a column (the pair is enabled where it is nonzero) or
        None.  Returns (n_missing, first_missing_row): the enabled pairs whose
        tuple is no key and the lowest such row, None when nothing is
        missing."""
        arity, n_tuples, table, values, sels = _lookup_tuple_lists(
            self._width, value_tuples, table_columns, count_column, selectors)
        ctx = context(device)
        n, first = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().mlh_trace_lookup_tuple_counts(
            ctx, ptr(self._matrix), self._height.bit_length() - 1, self._width, arity, table,
            n_tuples, values, sels, count_column, ctypes.byref(n), ctypes.byref(first)), ctx)
        return n.value, (None if first.value == 2 ** 64 - 1 else first.value)

    def lookup_tuple_multiplicities(self, value_tuples, table_columns, count_column,
                                    selectors=None, device=0):
        """lookup_tuple_counts for a lookup that must hold: ValueError naming
        the number of missing tuples and the first row with one."""
        n, first = self.lookup_tuple_counts(value_tuples, table_columns, count_column, selectors,
                                            device)
        if n:
            raise ValueError("%d looked-up tuple%s not in table columns %s, the first in row %d"
                             % (n, "" if n == 1 else "s", tuple(table_columns), first))


_NONE64, _NONE32 = 2 ** 64 - 1, 2 ** 32 - 1


class CheckResult:
    """What Trace.check and Trace.check_public return.  bad_rows: the rows on
    which anything fails; first_bad_row and first_bad_constraint: the lowest of
    them and the lowest constraint (column of the strip) failing there, None
    when clean; counts[c] / first_rows[c]: the failing rows of constraint c and
    the lowest of them (None when none); ok: nothing fails."""

    __slots__ = ("bad_rows", "first_bad_row", "first_bad_constraint", "counts", "first_rows")

    def __init__(self, bad_rows, first_bad_row, first_bad_constraint, counts, first_rows):
        self.bad_rows = bad_rows
        self.first_bad_row = None if first_bad_row == _NONE64 else first_bad_row
        self.first_bad_constraint = None if first_bad_constraint == _NONE32 else first_bad_constraint
        self.counts = list(counts)
        self.first_rows = [None if r == _NONE64 else r for r in first_rows]

    @property
    def ok(self):
        return self.bad_rows == 0

    def __repr__(self):
        return ("CheckResult(bad_rows=%r, first_bad_row=%r, first_bad_constraint=%r, counts=%r, "
                "first_rows=%r)" % (self.bad_rows, self.first_bad_row, self.first_bad_constraint,
                                    self.counts, self.first_rows))


def _check_arguments(width, program, randoms, shift_columns):
    """The shift list and the randoms of Trace.check, checked (ValueError) as
    mlh_trace_check checks them."""
    cols, randoms = [int(c) for c in shift_columns], list(randoms)
    for c in cols:
        if not 0 <= c < width:
            raise ValueError("source column %r outside the trace" % (c,))
    if width + len(cols) != program.width:
        raise ValueError("the program is %d columns wide, the trace %d and the shift list %d"
                         % (program.width, width, len(cols)))
    if len(randoms) != program.n_randoms:
        raise ValueError("the program takes %d randoms" % program.n_randoms)
    return cols, randoms


def trace_check_launch_info(program, log_height):
    """(threads per block, blocks) of mlh_trace_check."""
    t, b = ctypes.c_uint32(), ctypes.c_uint32()
    check(lib().mlh_trace_check_launch_info(program.h, log_height, ctypes.byref(t), ctypes.byref(b)))
    return t.value, b.value


LOOKUP_MAX_ARITY, LOOKUP_MAX_TUPLES, LOOKUP_NO_SELECTOR = 8, 16, 0xFFFFFFFF


def _lookup_tuple_lists(width, value_tuples, table_columns, count_column, selectors):
    """The column lists of a tuple lookup, checked (ValueError), as the arrays
    mlh_trace_lookup_tuple_counts takes: (arity, n_tuples, table, values,
    selectors or None)."""
    table = [int(c) for c in table_columns]
    tuples = [[int(c) for c in t] for t in value_tuples]
    arity, n_tuples = len(table), len(tuples)
    if not 1 <= arity <= LOOKUP_MAX_ARITY:
        raise ValueError("a tuple lookup has 1..%d table columns, not %d" % (LOOKUP_MAX_ARITY, arity))
    if not 1 <= n_tuples <= LOOKUP_MAX_TUPLES:
        raise ValueError("a tuple lookup has 1..%d value tuples, not %d"
                         % (LOOKUP_MAX_TUPLES, n_tuples))
    if arity * n_tuples > 32:
        raise ValueError("%d tuples of arity %d are more than 32 value columns" % (n_tuples, arity))
    if not 0 <= count_column < width:
        raise ValueError("count column %r outside the trace" % (count_column,))
    for c in table:
        if not 0 <= c < width:
            raise ValueError("table column %r outside the trace" % (c,))
        if c == count_column:
            raise ValueError("the count column %d is a table column" % c)
    if len(set(table)) != arity:
        raise ValueError("a table column occurs twice in %r" % (tuple(table),))
    for t in tuples:
        if len(t) != arity:
            raise ValueError("value tuple %r has not the table's arity %d" % (tuple(t), arity))
        for c in t:
            if not 0 <= c < width:
                raise ValueError("value column %r outside the trace" % (c,))
            if c in table:
                raise ValueError("the value column %d is a table column" % c)
            if c == count_column:
                raise ValueError("the count column %d is a value column" % c)
    sels = None
    if selectors is not None:
        sels = [LOOKUP_NO_SELECTOR if s is None else int(s) for s in selectors]
        if len(sels) != n_tuples:
            raise ValueError("%d selectors for %d value tuples" % (len(sels), n_tuples))
        for s in sels:
            if s != LOOKUP_NO_SELECTOR and not 0 <= s < width:
                raise ValueError("selector column %r outside the trace" % (s,))
            if s == count_column:
                raise ValueError("the count column %d is a selector" % s)
        sels = (ctypes.c_uint32 * n_tuples)(*sels)
    return (arity, n_tuples, (ctypes.c_uint32 * arity)(*table),
            (ctypes.c_uint32 * (arity * n_tuples))(*[c for t in tuples for c in t]), sels)


def lookup_tuple_counts_launch_info(log_height, n_tuples):
    """(threads per block, blocks of the count launch, log2 of the slots)."""
    t, b, s = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    check(lib().mlh_trace_lookup_tuple_counts_launch_info(log_height, n_tuples, ctypes.byref(t),
                                                          ctypes.byref(b), ctypes.byref(s)))
    return t.value, b.value, s.value


def tuple_key(columns, alpha):
    """var(c0) + alpha * (var(c1) + alpha * (...)): a tuple's components
    compressed with ``alpha`` (an Expr such as ``rand(1)``, or an int), so that
    a phase-2 fill and its constraint spell the key of a tuple lookup once."""
    cols = [int(c) for c in columns]
    if not cols:
        raise ValueError("a tuple key needs a column")
    alpha = Expr.wrap(alpha)
    e = var(cols[-1])
    for c in reversed(cols[:-1]):
        e = var(c) + alpha * e
    return e


def _lookup_mask(width, value_columns, table_column, count_column):
    """The value-column mask of a lookup, its columns checked (ValueError)."""
    mask = 0
    for j in value_columns:
        if not 0 <= j < width:
            raise ValueError("value column %r outside the trace" % (j,))
        mask |= 1 << j
    if not mask:
        raise ValueError("a lookup needs a value column")
    for name, j in (("table", table_column), ("count", count_column)):
        if not 0 <= j < width:
            raise ValueError("%s column %r outside the trace" % (name, j))
        if (mask >> j) & 1:
            raise ValueError("the %s column %d is a value column" % (name, j))
    if table_column == count_column:
        raise ValueError("the table column and the count column are both %d" % table_column)
    return mask


def lookup_counts_launch_info(log_height, n_value_columns):
    """(threads per block, blocks of the count launch, log2 of the slots)."""
    t, b, s = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    check(lib().mlh_trace_lookup_counts_launch_info(log_height, n_value_columns, ctypes.byref(t),
                                                    ctypes.byref(b), ctypes.byref(s)))
    return t.value, b.value, s.value


SCAN_OPS = {"add": 0, "mul": 1}


def _scan_arrays(scans, width):
    """(ops, sources, destinations, inits) of a list of (op, src, dst, init),
    checked as mlh_trace_scan checks them."""
    scans = list(scans)
    if not 1 <= len(scans) <= 8:
        raise ValueError("1 to 8 scans in one call, not %d" % len(scans))
    ops, src, dst, inits = [], [], [], []
    for op, s, d, init in scans:
        if op not in SCAN_OPS:
            raise ValueError("scan op %r is neither 'add' nor 'mul'" % (op,))
        for name, j in (("source", s), ("destination", d)):
            if not 0 <= j < width:
                raise ValueError("%s column %r outside the trace" % (name, j))
        if d in dst:
            raise ValueError("two scans write column %d" % d)
        ops.append(SCAN_OPS[op])
        src.append(s)
        dst.append(d)
        inits.append(init)
    return ops, src, dst, inits


def trace_scan_launch_info(log_height, width, n_scans):
    """(threads per block, consecutive rows per thread, blocks) of mlh_trace_scan."""
    t, k, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    check(lib().mlh_trace_scan_launch_info(log_height, width, n_scans, ctypes.byref(t),
                                           ctypes.byref(k), ctypes.byref(b)))
    return t.value, k.value, b.value


SORT_MAX_KEYS, SORT_MAX_COPIES, SORT_NO_COLUMN = 4, 16, 0xFFFFFFFF


def _sort_arrays(keys, copies, perm_column, width):
    """(keys, sources, destinations, perm column or SORT_NO_COLUMN) of a sort,
    checked as mlh_trace_sort checks them."""
    keys = [int(k) for k in keys]
    copies = [(int(s), int(d)) for s, d in copies]
    if not 1 <= len(keys) <= SORT_MAX_KEYS:
        raise ValueError("1 to %d key columns, not %d" % (SORT_MAX_KEYS, len(keys)))
    if len(copies) > SORT_MAX_COPIES:
        raise ValueError("at most %d copies in one call, not %d" % (SORT_MAX_COPIES, len(copies)))
    if not copies and perm_column is None:
        raise ValueError("a sort needs an output: a copy or a perm_column")
    src, dst = [s for s, _ in copies], [d for _, d in copies]
    written = dst + ([int(perm_column)] if perm_column is not None else [])
    for name, cols in (("key", keys), ("source", src), ("destination", written)):
        for j in cols:
            if not 0 <= j < width:
                raise ValueError("%s column %r outside the trace" % (name, j))
    if len(set(written)) != len(written):
        raise ValueError("destination columns and perm_column must be pairwise distinct")
    both = set(written) & (set(keys) | set(src))
    if both:
        raise ValueError("column %d is written and is a key or a source" % min(both))
    return keys, src, dst, SORT_NO_COLUMN if perm_column is None else int(perm_column)


def trace_sort_launch_info(log_height, width, n_keys):
    """(threads per block, rows per thread, blocks) of mlh_trace_sort."""
    t, k, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    check(lib().mlh_trace_sort_launch_info(log_height, width, n_keys, ctypes.byref(t),
                                           ctypes.byref(k), ctypes.byref(b)))
    return t.value, k.value, b.value


def trace_column_sum(dev_matrix, width, columns, device=0):
    """sum_i sum_{j in columns} matrix[i * width + j] (mlh_trace_column_sum):
    the column_sum of a two-phase proof for columns = layout.sum_columns."""
    n = dev_matrix.shape[0]
    assert width >= 1 and n % width == 0
    height = n // width
    assert height & (height - 1) == 0 and height > 0
    mask = 0
    for j in columns:
        if not 0 <= j < width:
            raise ValueError("column %r outside the trace" % (j,))
        mask |= 1 << j
    ctx = context(device)
    out = (ctypes.c_uint8 * 16)()
    check(lib().mlh_trace_column_sum(ctx, ptr(dev_matrix), height.bit_length() - 1, width, mask,
                                     out), ctx)
    return fe_from_bytes(out)


def trace_columns(dev_matrix, width, device=0, columns=None):
    """The row-major (height * width, 4) trace as its width column MLEs,
    column-major: a new tensor, column j at rows [j * height, (j + 1) * height)
    (mlh_trace_columns).  columns = (col0, ncols): those columns only
    (mlh_trace_columns_range)."""
    n = dev_matrix.shape[0]
    assert width >= 1 and n % width == 0
    height = n // width
    assert height & (height - 1) == 0 and height > 0
    ctx = context(device)
    if columns is not None:
        col0, ncols = columns
        out = empty(height * ncols, device)
        check(lib().mlh_trace_columns_range(ctx, ptr(dev_matrix), height.bit_length() - 1, width,
                                            col0, ncols, ptr(out)), ctx)
        return out
    out = empty(n, device)
    check(lib().mlh_trace_columns(ctx, ptr(dev_matrix), height.bit_length() - 1, width, ptr(out)),
          ctx)
    return out


# ---- field ops on device vectors (field.rs:66-118) ----------------------------

def _field2(fn, a, b, out, device):
    ctx = context(device)
    out = empty(a.shape[0], device) if out is None else out
    check(fn(ctx, ptr(a), ptr(b), ptr(out), a.shape[0]), ctx)
    return out


def field_add(a, b, out=None, device=0):
    return _field2(lib().mlh_field_add, a, b, out, device)


def field_sub(a, b, out=None, device=0):
    return _field2(lib().mlh_field_sub, a, b, out, device)


def field_mul(a, b, out=None, device=0):
    return _field2(lib().mlh_field_mul, a, b, out, device)


def field_neg(a, out=None, device=0):
    ctx = context(device)
    out = empty(a.shape[0], device) if out is None else out
    check(lib().mlh_field_neg(ctx, ptr(a), ptr(out), a.shape[0]), ctx)
    return out


def field_scale(a, c, out=None, device=0):
    ctx = context(device)
    out = empty(a.shape[0], device) if out is None else out
    check(lib().mlh_field_scale(ctx, ptr(a), fe_bytes(c), ptr(out), a.shape[0]), ctx)
    return out


def field_inv(a, out=None, device=0):
    """out[i] = 1 / a[i], zero -> zero (mlh_field_inv); out may be a itself."""
    ctx = context(device)
    out = empty(a.shape[0], device) if out is None else out
    check(lib().mlh_field_inv(ctx, ptr(a), ptr(out), a.shape[0]), ctx)
    return out


class Commitment:
    """trace.rs:40-48 made real: the batched-PCS commit phase over the trace's
    columns (mlh_trace_commitment).  Owns the column evaluations, the RS codes
    and the batch tree on the device; the trace is not modified."""

    def __init__(self, handle, device):
        self.h = handle
        self._device = device
        self.width = lib().mlh_trace_commitment_width(handle)
        self.log_height = lib().mlh_trace_commitment_log_height(handle)

    def __del__(self):
        try:
            lib().mlh_trace_commitment_destroy(self.h)
        except Exception:
            pass

    @staticmethod
    def new(trace, device=0, columns=None):  # trace.rs:44-47
        """columns = (col0, ncols): a commitment to those columns only
        (mlh_trace_commit_range)."""
        ctx = context(device)
        h = ctypes.c_void_p()
        L = trace.height().bit_length() - 1
        if columns is not None:
            check(lib().mlh_trace_commit_range(ctx, ptr(trace.matrix()), L, trace.width(),
                                               columns[0], columns[1], ctypes.byref(h)), ctx)
        else:
            check(lib().mlh_trace_commit(ctx, ptr(trace.matrix()), L, trace.width(),
                                         ctypes.byref(h)), ctx)
        return Commitment(h.value, device)

    def root(self):
        out = (ctypes.c_uint8 * 32)()
        check(lib().mlh_trace_commitment_root(self.h, out))
        return bytes(out)


def _program_of(constraints, layout):
    return Program(compile_program(constraints.constraints(), layout.columns, layout.randoms,
                                   constraints.degree()))


def _shifted_program_of(constraints, layout):
    """-> (Program, shift list): compile_shifted of the constraint set."""
    wire, shifts = compile_shifted(constraints.constraints(), layout.columns, layout.randoms,
                                   constraints.degree())
    return Program(wire), shifts


class _ProofHolder:
    """What SystemProof and PhasedSystemProof share: the header, the buffers of
    the sumcheck polynomials and of Trace::evaluate(rs) behind the C struct
    ``c``, and their views."""

    def __init__(self, c, log_height, width, degree):
        self.log_height, self.width, self.degree = log_height, width, degree
        self._polys = (ctypes.c_uint8 * (16 * (degree + 1) * log_height))()
        self._output = (ctypes.c_uint8 * (16 * width))()
        self.c = c
        c.log_height, c.width, c.degree = log_height, width, degree
        c.sumcheck_polys = ctypes.cast(self._polys, ctypes.c_void_p)
        c.output = ctypes.cast(self._output, ctypes.c_void_p)

    def _sync(self):  # the struct holds copies of the nested ones
        for p, c in self._nested():
            p.c = c
            p.fri_proof.c = c.fri

    @property
    def sumcheck_polynomials(self):
        D = self.degree + 1
        flat = _split(self._polys, D * self.log_height)
        return [flat[D * k:D * k + D] for k in range(self.log_height)]

    @property
    def output(self):
        return _split(self._output, self.width)


class SystemProof(_ProofHolder):
    """mlh_system_proof: the sumcheck polynomials, Trace::evaluate(rs) and the
    batched-PCS opening of the committed columns at rs."""

    def __init__(self, log_height, width, degree):
        super().__init__(_lib.SystemProofC(), log_height, width, degree)
        self.pcs = BatchedPCSProof(log_height, width)
        self.c.pcs = self.pcs.c

    def _nested(self):
        return [(self.pcs, self.c.pcs)]

    @property
    def commitment(self):
        return bytes(self.c.pcs.fri.batch_commitment)

    def verify(self, transcript, constraints, layout, total_sum):
        """mlh_system_verify, host only: True iff accepted.  The transcript
        is the one the prover started from; it is advanced only on True."""
        prog = _program_of(constraints, layout)
        return lib().mlh_system_verify(prog.h, self.log_height, fe_bytes(total_sum),
                                       ctypes.byref(self.c), transcript.h) == 0


def _column_mask(layout):
    m = 0
    for j in layout.sum_columns:
        if not 0 <= j < layout.columns:
            raise ValueError("sum column %r outside the trace" % (j,))
        m |= 1 << j
    return m


class PhasedSystemProof(_ProofHolder):
    """mlh_phased_proof: the sumcheck polynomials, Trace::evaluate(rs) and the
    openings of the two commitments (columns [0, P) and [P, W)) at rs."""

    def __init__(self, log_height, width, degree, pre_random_columns, sum_column_mask):
        super().__init__(_lib.PhasedProofC(), log_height, width, degree)
        self.pre_random_columns, self.sum_column_mask = pre_random_columns, sum_column_mask
        P = pre_random_columns
        self.pcs = [BatchedPCSProof(log_height, P)]
        if P < width:
            self.pcs.append(BatchedPCSProof(log_height, width - P))
        self.c.pre_random_columns, self.c.sum_column_mask = P, sum_column_mask
        for i, p in enumerate(self.pcs):
            self.c.pcs[i] = p.c

    def _nested(self):
        return [(p, self.c.pcs[i]) for i, p in enumerate(self.pcs)]

    @property
    def commitments(self):
        return [bytes(self.c.pcs[i].fri.batch_commitment) for i in range(len(self.pcs))]

    def verify(self, transcript, constraints, layout, total_sum, column_sum):
        """mlh_system_verify_phased, host only: True iff accepted.  The
        transcript is the one the prover started from; it is advanced only on
        True."""
        prog = _program_of(constraints, layout)
        return lib().mlh_system_verify_phased(prog.h, self.log_height, layout.pre_random_columns,
                                              _column_mask(layout), fe_bytes(total_sum),
                                              fe_bytes(column_sum), ctypes.byref(self.c),
                                              transcript.h) == 0


class ShiftedSystemProof(_ProofHolder):
    """mlh_shifted_proof: the phased proof over the extended trace (output has
    width + K elements), the shift reduction's polynomials, Trace::evaluate(rs')
    and the openings of both commitments at rs and at rs'."""

    def __init__(self, log_height, width, degree, pre_random_columns, sum_column_mask,
                 shift_columns, n_public=0):
        super().__init__(_lib.ShiftedProofC(), log_height, width, degree)
        self.n_public = n_public
        self.pre_random_columns, self.sum_column_mask = pre_random_columns, sum_column_mask
        self.shift_columns = [int(c) for c in shift_columns]
        K, P, c = len(self.shift_columns), pre_random_columns, self.c
        self._output = (ctypes.c_uint8 * (16 * (width + K)))()
        self._shift_polys = (ctypes.c_uint8 * (32 * log_height))()
        self._output2 = (ctypes.c_uint8 * (16 * width))()
        c.output = ctypes.cast(self._output, ctypes.c_void_p)
        c.shift_polys = ctypes.cast(self._shift_polys, ctypes.c_void_p)
        c.output2 = ctypes.cast(self._output2, ctypes.c_void_p)
        c.pre_random_columns, c.sum_column_mask, c.n_shifts = P, sum_column_mask, K
        for k, col in enumerate(self.shift_columns):
            c.shift_columns[k] = col
        committed = width - n_public  # the openings leave the public columns out
        widths = [P] + ([committed - P] if P < committed else [])
        self.pcs = [BatchedPCSProof(log_height, w) for w in widths]
        self.pcs_shift = [BatchedPCSProof(log_height, w) for w in widths] if K else []
        for i, p in enumerate(self.pcs):
            c.pcs[i] = p.c
        for i, p in enumerate(self.pcs_shift):
            c.pcs_shift[i] = p.c

    def _nested(self):
        return ([(p, self.c.pcs[i]) for i, p in enumerate(self.pcs)]
                + [(p, self.c.pcs_shift[i]) for i, p in enumerate(self.pcs_shift)])

    @property
    def commitments(self):
        return [bytes(self.c.pcs[i].fri.batch_commitment) for i in range(len(self.pcs))]

    @property
    def output(self):
        return _split(self._output, self.width + len(self.shift_columns))

    @property
    def shift_polynomials(self):
        if not self.shift_columns:
            return []
        flat = _split(self._shift_polys, 2 * self.log_height)
        return [flat[2 * k:2 * k + 2] for k in range(self.log_height)]

    @property
    def output2(self):
        return _split(self._output2, self.width) if self.shift_columns else []

    def verify(self, transcript, constraints, layout, total_sum, column_sum, public=None):
        """mlh_system_verify_public (without public columns:
        mlh_system_verify_shifted), host only: True iff accepted.  The
        constraint set is the prover's, with its ``nxt`` columns; the transcript
        is the one the prover started from and is advanced only on True.
        public (a PublicColumns; None: the layout's): the verifier's own spec of
        the public columns."""
        prog, shifts = _shifted_program_of(constraints, layout)
        arr = (ctypes.c_uint32 * max(len(shifts), 1))(*shifts)
        if public is None:
            public = getattr(layout, "public_columns", None)
        return lib().mlh_system_verify_public(prog.h, self.log_height, layout.pre_random_columns,
                                              _column_mask(layout), arr, len(shifts),
                                              public.h if public is not None and len(public) else None,
                                              fe_bytes(total_sum), fe_bytes(column_sum),
                                              ctypes.byref(self.c), transcript.h) == 0


class PhasedProver:
    """System::prover for a layout with pre_random_columns / sum_columns
    (system.rs:17-30, 56-72): holds the commitment to columns [0, P) and the
    trace randoms drawn after it; ``prove`` commits to the other columns of
    the matrix as it then stands.  With public columns in the layout (its last
    ones) the strip is filled here, before the first commitment, the
    commitments cover the columns below it, and ``prove`` runs
    mlh_system_prove_public."""

    def __init__(self, transcript, constraints, layout, trace, device=0):
        P, W = layout.pre_random_columns, layout.columns
        self._public = getattr(layout, "public_columns", None)
        self._committed = W - (len(self._public) if self._public is not None else 0)
        if not 1 <= P <= self._committed or W != trace.width():
            raise ValueError("pre_random_columns must be in 1..columns less the public ones, "
                             "columns the trace's width")
        self._constraints, self._layout, self._trace, self._device = constraints, layout, trace, device
        self._mask = _column_mask(layout)
        self.program, self.shift_columns = _shifted_program_of(constraints, layout)
        if self._public is not None:
            trace.fill_public(self._public, device)
        self._com1 = Commitment.new(trace, device, columns=(0, P))
        out = (ctypes.c_uint8 * (16 * max(layout.randoms, 1)))()
        head = transcript
        if self._public is not None:  # step 0: the spec's digest comes before the root
            head = transcript.clone()
            head.absorb(self._public.digest)
        check(lib().mlh_system_trace_randoms(head.h, self._com1.root(), layout.randoms, out))
        self.randoms = _split(out, layout.randoms)
        self._entry = transcript.random()

    def commitment(self):
        return self._com1

    def fill(self, assignments):
        """Fill columns at and above pre_random_columns in place with
        {column: Expr} over the row and ``self.randoms`` (mlh_trace_fill).  A
        written column of commitment 1 would make the proof unprovable:
        ValueError."""
        lay = self._layout
        prog = FillProgram(compile_fill(assignments, lay.columns, lay.randoms))
        if prog.output_mask & ((1 << lay.pre_random_columns) - 1):
            raise ValueError("fill writes a column below pre_random_columns (%d), which "
                             "commitment 1 already holds" % lay.pre_random_columns)
        return self._trace.fill(prog, self.randoms, self._device)

    def scan(self, scans):
        """``Trace.scan`` on the prover's trace: running sums and products
        into columns at and above pre_random_columns and below the public
        strip; returns the totals.  A destination that commitment 1 already
        holds, or a public column (which the verifier derives): ValueError."""
        lay = self._layout
        scans = list(scans)
        for _, _, d, _ in scans:
            if 0 <= d < lay.pre_random_columns:
                raise ValueError("scan writes column %d below pre_random_columns (%d), which "
                                 "commitment 1 already holds" % (d, lay.pre_random_columns))
            if self._committed <= d < lay.columns:
                raise ValueError("scan writes the public column %d" % d)
        return self._trace.scan(scans, self._device)

    def sort(self, keys, copies, perm_column=None):
        """``Trace.sort`` on the prover's trace: sorted copies into columns at
        and above pre_random_columns and below the public strip; returns the
        number of digit passes.  A destination (or perm_column) that
        commitment 1 already holds, or a public column: ValueError."""
        lay = self._layout
        copies = list(copies)
        for d in [d for _, d in copies] + ([perm_column] if perm_column is not None else []):
            if 0 <= d < lay.pre_random_columns:
                raise ValueError("sort writes column %d below pre_random_columns (%d), which "
                                 "commitment 1 already holds" % (d, lay.pre_random_columns))
            if self._committed <= d < lay.columns:
                raise ValueError("sort writes the public column %d" % d)
        return self._trace.sort(keys, copies, perm_column, self._device)

    def check(self):
        """The witness check of the trace as it stands, before ``prove``: the
        prover's own program with ``self.shift_columns`` and ``self.randoms``
        (Trace.check), and with public columns in the layout the strip against
        its spec (Trace.check_public).  Returns (constraints, public), each a
        CheckResult, public None without public columns.  No transcript is
        touched."""
        res = self._trace.check(self.program, self.randoms, self.shift_columns, self._device)
        pub = None
        if self._public is not None:
            pub = self._trace.check_public(self._public, self._device)
        return res, pub

    def prove(self, transcript, total_sum, column_sum=None):
        """mlh_system_prove_phased on a clone of the trace's matrix.
        column_sum = None: the sum of layout.sum_columns as the matrix stands
        (mlh_trace_column_sum).  The value proved is kept in ``self.column_sum``."""
        if transcript.random() != self._entry:
            raise ValueError("prove needs the transcript in the state phased_prover was given")
        ctx = context(self._device)
        t, lay = self._trace, self._layout
        P, W = lay.pre_random_columns, lay.columns
        if column_sum is None:
            column_sum = trace_column_sum(t.matrix(), W, lay.sum_columns, self._device)
        self.column_sum = column_sum
        C = self._committed
        com2 = Commitment.new(t, self._device, columns=(P, C - P)) if P < C else None
        if self.shift_columns or self._public is not None:
            # a shifted constraint set or public columns: the trace itself is not modified
            K = len(self.shift_columns)
            p = ShiftedSystemProof(self._com1.log_height, W, self._constraints.degree(), P,
                                   self._mask, self.shift_columns, W - C)
            check(lib().mlh_system_prove_public(ctx, self.program.h, self._com1.h,
                                                com2.h if com2 else None, self._mask,
                                                (ctypes.c_uint32 * max(K, 1))(*self.shift_columns), K,
                                                self._public.h if self._public is not None else None,
                                                ptr(t.matrix()), fe_bytes(total_sum),
                                                fe_bytes(column_sum), transcript.h,
                                                ctypes.byref(p.c)), ctx)
            p._sync()
            return p
        p = PhasedSystemProof(self._com1.log_height, W, self._constraints.degree(), P, self._mask)
        work = t.matrix().clone()
        check(lib().mlh_system_prove_phased(ctx, self.program.h, self._com1.h,
                                            com2.h if com2 else None, self._mask, ptr(work),
                                            fe_bytes(total_sum), fe_bytes(column_sum), transcript.h,
                                            ctypes.byref(p.c)), ctx)
        p._sync()
        return p


class ChallengeSet:
    """system.rs:32-36,131-159, with the constraint mask of System::new
    (:90-95) from the same call (mlh_system_challenges)."""

    def __init__(self, transcript, num_randoms, num_constraints, log_num_rows):
        log_nc = max(num_constraints - 1, 0).bit_length()
        row = (ctypes.c_uint8 * (16 * max(log_num_rows, 1)))()
        trace = (ctypes.c_uint8 * (16 * max(num_randoms, 1)))()
        cons = (ctypes.c_uint8 * (16 * max(log_nc, 1)))()
        mask = (ctypes.c_uint8 * (16 * max(num_constraints, 1)))()
        check(lib().mlh_system_challenges(transcript.h, log_num_rows, num_randoms, num_constraints,
                                          row, trace, cons, mask))
        self._row = _split(row, log_num_rows)
        self._trace = _split(trace, num_randoms)
        self._constraint = _split(cons, log_nc)
        self.mask = _split(mask, num_constraints)

    def row(self):
        return self._row

    def trace(self):
        return self._trace

    def constraint(self):
        return self._constraint


class SumcheckTables:
    """sumcheck.rs:10-15: the matrix, its width and height, delta."""

    def __init__(self, matrix, width, height, delta):
        self.matrix = matrix
        self.width = width
        self.height = height
        self.delta = delta


class System:
    """system.rs:8-129 with the sumcheck methods of sumcheck.rs:21-125."""

    def __init__(self, transcript, constraints, layout, log_num_rows, trace, device=0):
        self._constraints = constraints
        self._layout = layout
        self._trace = trace
        self._device = device
        self._commitment = None
        n = len(constraints.constraints())
        self._challenges = ChallengeSet(transcript, layout.randoms, n, log_num_rows)
        self._constraint_mask = self._challenges.mask
        self.program = _program_of(constraints, layout)

    @staticmethod
    def prover(transcript, constraints, layout, trace, device=0):  # system.rs:56-72
        return System(transcript, constraints, layout, trace.height().bit_length() - 1, trace,
                      device)

    @staticmethod
    def committed_prover(transcript, constraints, layout, trace, device=0):
        """system.rs:56-72 with the commitment made: commits to the trace, and
        draws the challenges after the root on a clone of ``transcript``, which
        is left as it was -- ``prove`` absorbs the root into it.  (``prover``
        keeps the reference's behaviour, where Commitment::new is a TODO and
        nothing is absorbed.)"""
        com = Commitment.new(trace, device)
        t = transcript.clone()
        t.absorb(com.root())
        s = System(t, constraints, layout, trace.height().bit_length() - 1, trace, device)
        s._commitment = com
        s._entry = transcript.random()
        return s

    @staticmethod
    def phased_prover(transcript, constraints, layout, trace, device=0):
        """The two-phase prover: commits to columns [0, pre_random_columns) of
        the trace and exposes ``.randoms``; ``transcript`` is left as it was
        (``.prove`` absorbs).  The caller then fills the other columns of the
        trace's matrix in place and calls ``.prove(transcript, total_sum,
        column_sum)``."""
        return PhasedProver(transcript, constraints, layout, trace, device)

    def commitment(self):
        return self._commitment

    def prove(self, transcript, total_sum):
        """mlh_system_prove on a clone of the trace's matrix: root, challenges,
        sumcheck, opening.  ``transcript`` must be in the state
        ``committed_prover`` saw."""
        if transcript.random() != self._entry:
            raise ValueError("prove needs the transcript in the state committed_prover was given")
        ctx = context(self._device)
        com, t = self._commitment, self._trace
        p = SystemProof(com.log_height, com.width, self._constraints.degree())
        work = t.matrix().clone()
        check(lib().mlh_system_prove(ctx, self.program.h, com.h, ptr(work), fe_bytes(total_sum),
                                     transcript.h, ctypes.byref(p.c)), ctx)
        p._sync()
        return p

    @staticmethod
    def verifier(transcript, constraints, layout, log_num_rows, device=0):  # system.rs:39-54
        return System(transcript, constraints, layout, log_num_rows, None, device)

    def num_columns(self):
        return self._layout.columns

    def constraints(self):
        return self._constraints

    def constraint_mask(self):
        return self._constraint_mask

    def challenges(self):
        return self._challenges

    def trace(self):
        return self._trace

    def evaluate_composition(self, outputs):  # evaluation.rs:5-11
        assert len(outputs) == self.num_columns()
        return self.program.evaluate(outputs, self._challenges.trace(), self._constraint_mask)

    def build_tables(self):
        """sumcheck.rs:22-38: a clone of the trace's matrix and delta = the eq
        table of the row challenges (mlh_eq_table)."""
        t = self._trace
        delta = eq_table(self._challenges.row(), self._device)
        return SumcheckTables(t.matrix().clone(), t.width(), t.height(), delta)

    def compute_sumcheck_polynomials(self, transcript: Transcript, tables, total_sum):
        """sumcheck.rs:40-53 -> ([nonzero coefficients c1..cD] per round, [r]);
        the tables are folded in place down to height 1."""
        ctx = context(self._device)
        n = tables.height.bit_length() - 1
        D = self._constraints.degree() + 1
        polys = (ctypes.c_uint8 * (16 * D * max(n, 1)))()
        rs = (ctypes.c_uint8 * (16 * max(n, 1)))()
        check(lib().mlh_cs_sumcheck_prove(ctx, self.program.h, tables.width, ptr(tables.matrix),
                                          ptr(tables.delta), n, _elems(self._challenges.trace()),
                                          _elems(self._constraint_mask), fe_bytes(total_sum),
                                          transcript.h, polys, rs), ctx)
        tables.height = 1
        flat = _split(polys, D * n)
        return [flat[D * k:D * k + D] for k in range(n)], _split(rs, n)

    def verify_with_evaluations(self, transcript: Transcript, pols, total_sum, output):
        """sumcheck.rs:91-124 on the host; raises MlhError (MLH_ERR_VERIFY)
        where the reference asserts."""
        n = len(pols)
        flat = [c for p in pols for c in p]
        check(lib().mlh_cs_sumcheck_verify(self.program.h, n, _elems(self._challenges.row()),
                                           _elems(self._challenges.trace()),
                                           _elems(self._constraint_mask), fe_bytes(total_sum),
                                           _elems(flat), _elems(output), transcript.h))

    def verify_sumcheck_debug(self, transcript: Transcript, pols, total_sum):
        """sumcheck.rs:55-89: as verify_with_evaluations with the output taken
        from the prover's own trace at the challenges, which a clone of the
        transcript replays first."""
        t = transcript.clone()
        rs = []
        for p in pols:
            for c in p:
                t.absorb(int(c).to_bytes(16, "little"))
            rs.append(t.next_challenge())
        output = self._trace.evaluate(rs, self._device)
        self.verify_with_evaluations(transcript, pols, total_sum, output)
