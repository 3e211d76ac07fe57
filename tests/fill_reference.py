"""Plain-Python model of fill programs (include/mlhip.h): interprets the wire
bytes row by row with pow(x, M - 2, M).  Shares nothing with libmlhip or with
compile_fill's emitter beyond the documented format; it assumes a valid
program (the decoder's rejections are tested against hand-made bytes)."""
import struct

M = 2**128 - 45 * 2**40 + 1

ADD, SUB, MUL, NEG, INV = range(5)
COL, RAND, CONST, TEMP = range(4)


def wire(width, n_randoms, consts, n_temps, instrs, outs, reserved=0):
    """instrs: (op, dst, (kind, index), (kind, index)); outs: (column, kind, index)."""
    b = struct.pack("<7I", width, n_randoms, len(consts), n_temps, len(instrs), len(outs), reserved)
    for c in consts:
        b += int(c).to_bytes(16, "little")
    for op, dst, a, bb in instrs:
        b += bytes([op, dst, a[0], a[1], bb[0], bb[1], 0, 0])
    for col, kind, index in outs:
        b += bytes([col, kind, index, 0])
    return b


def parse(w):
    width, n_randoms, n_consts, n_temps, n_instr, n_outputs, _ = struct.unpack_from("<7I", w, 0)
    q = 28
    consts = [int.from_bytes(w[q + 16 * i:q + 16 * i + 16], "little") for i in range(n_consts)]
    q += 16 * n_consts
    instrs = [tuple(w[q + 8 * i:q + 8 * i + 6]) for i in range(n_instr)]
    q += 8 * n_instr
    outs = [tuple(w[q + 4 * i:q + 4 * i + 3]) for i in range(n_outputs)]
    assert q + 4 * n_outputs == len(w)
    return dict(width=width, n_randoms=n_randoms, consts=consts, n_temps=n_temps, instrs=instrs,
                outs=outs)


def fill_row(p, row, randoms):
    """The row after the fill: column operands read ``row``."""
    temps = [0] * max(p["n_temps"], 1)

    def get(kind, index):
        return (row, randoms, p["consts"], temps)[kind][index]

    for op, dst, ak, ai, bk, bi in p["instrs"]:
        a = get(ak, ai)
        if op == ADD:
            r = (a + get(bk, bi)) % M
        elif op == SUB:
            r = (a - get(bk, bi)) % M
        elif op == MUL:
            r = a * get(bk, bi) % M
        elif op == NEG:
            r = -a % M
        else:
            r = pow(a, M - 2, M)
        temps[dst] = r
    vals = [get(k, i) for _, k, i in p["outs"]]
    out = list(row)
    for (col, _, _), v in zip(p["outs"], vals):
        out[col] = v
    return out


def fill_matrix(w, matrix, randoms):
    """Row-major flat matrix -> the filled flat matrix."""
    p = parse(w)
    W = p["width"]
    out = []
    for i in range(0, len(matrix), W):
        out += fill_row(p, matrix[i:i + W], randoms)
    return out


# ---- the programs the CPU and GPU tests share (hand-written wire bytes) ----------

# the lookup pair: col3 = 1 / (rand0 - col0), col4 = -col2 / (rand0 - col1)
LOOKUP = wire(5, 1, [], 3,
              [(SUB, 0, (RAND, 0), (COL, 0)), (INV, 0, (TEMP, 0), (0, 0)),
               (NEG, 1, (COL, 2), (0, 0)), (SUB, 2, (RAND, 0), (COL, 1)),
               (INV, 2, (TEMP, 2), (0, 0)), (MUL, 2, (TEMP, 1), (TEMP, 2))],
              [(3, TEMP, 0), (4, TEMP, 2)])

# no INV: col2 = col0 * col1 (a product column), width 3
PRODUCT = wire(3, 0, [], 1, [(MUL, 0, (COL, 0), (COL, 1))], [(2, TEMP, 0)])

# an output that reads its own old column: col1 = col1 * col0 + rand0
SELF = wire(2, 1, [], 1, [(MUL, 0, (COL, 1), (COL, 0)), (ADD, 0, (TEMP, 0), (RAND, 0))],
            [(1, TEMP, 0)])

# width 2, one INV: col1 = 1 / (rand0 - col0)
INV2 = wire(2, 1, [], 1, [(SUB, 0, (RAND, 0), (COL, 0)), (INV, 0, (TEMP, 0), (0, 0))],
            [(1, TEMP, 0)])


def _wide16():
    """Width 32, 16 INVs: col[16 + v] = (col[v] + 7) / (rand0 - col[v]) for v < 15, and
    col31 = col15 + 1 / (rand1 * col15 - 3): temps reused after tainted values."""
    ins, outs = [], []
    for v in range(15):
        ins += [(SUB, 0, (RAND, 0), (COL, v)), (INV, 1, (TEMP, 0), (0, 0)),
                (ADD, 0, (COL, v), (CONST, 0)), (MUL, 2 + v, (TEMP, 0), (TEMP, 1))]
        outs.append((16 + v, TEMP, 2 + v))
    # temp 1 held an inverse and is written again before it feeds an INV
    ins += [(MUL, 1, (RAND, 1), (COL, 15)), (SUB, 1, (TEMP, 1), (CONST, 1)),
            (INV, 0, (TEMP, 1), (0, 0)), (ADD, 17, (COL, 15), (TEMP, 0))]
    outs.append((31, TEMP, 17))
    return wire(32, 2, [7, 3], 18, ins, outs)


WIDE16 = _wide16()

# zero -> zero: col1 = inv(const 0) + inv(col0) (col0 holds zero in some rows), col2 = rand0
ZEROS = wire(3, 1, [0], 2,
             [(INV, 0, (CONST, 0), (0, 0)), (INV, 1, (COL, 0), (0, 0)),
              (ADD, 0, (TEMP, 0), (TEMP, 1))],
             [(1, TEMP, 0), (2, RAND, 0)])
