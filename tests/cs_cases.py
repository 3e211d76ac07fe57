"""The constraint systems of the constraint-system sumcheck tests: each as a
constraint program (wire bytes, built with multilinear_amd.constraint_system)
and, independently, as the Python callables tests/cs_reference.py takes.
Shared by the CPU tests (host interpreter against the callables) and the GPU
tests (device prover against the model)."""
import random

from multilinear_amd.constraint_system import (COL, OP_ADD, OP_MUL, OP_NEG, TEMP, compile_program,
                                               encode_program, rand, var)
from oracle import field as F

M = F.M


class Case:
    def __init__(self, name, log_height, width, randoms, degree, wire, fns, seed=b""):
        self.name = name
        self.log_height = log_height
        self.width = width
        self.randoms = randoms
        self.degree = degree
        self.wire = wire
        self.fns = fns
        self.seed = seed  # absorbed before the challenges are drawn

    def matrix(self):
        r = random.Random("cs-" + self.name)
        return [r.randrange(M) for _ in range(self.width << self.log_height)]


def pythagorean_matrix():
    """16 Pythagorean triples by Euclid's formula (a, b, c) = (m^2 - n^2, 2mn,
    m^2 + n^2), m > n >= 1, and a + b as the fourth column."""
    rows = []
    m = 2
    while len(rows) < 16:
        for n in range(1, m):
            if len(rows) < 16:
                a, b, c = m * m - n * n, 2 * m * n, m * m + n * n
                rows.append([a, b, c, a + b])
        m += 1
    return [F.from_i64(v) for row in rows for v in row]


def pythagorean_exprs():
    return [var(0) * var(0) + var(1) * var(1) - var(2) * var(2), var(0) + var(1) - var(3)]


PYTHAGOREAN_FNS = [
    lambda x, r: (x[0] * x[0] + x[1] * x[1] - x[2] * x[2]) % M,
    lambda x, r: (x[0] + x[1] - x[3]) % M,
]


def _wide32_wire():
    """Raw program holding the maximum temp count: t_i = x_i * x_{i+1 mod 32}
    for all 32 temps, summed into t0 (dst == first operand), then t1 reused
    for -(t31)."""
    ins = [(OP_MUL, i, (COL, i), (COL, (i + 1) % 32)) for i in range(32)]
    ins += [(OP_ADD, 0, (TEMP, 0), (TEMP, i)) for i in range(1, 32)]
    ins += [(OP_NEG, 1, (TEMP, 31), (0, 0))]
    return encode_program(32, 0, [], 32, ins, [(TEMP, 0), (TEMP, 1)], 2)


def cases():
    out = []
    out.append(Case("lin1", 1, 1, 0, 1, compile_program([var(0) + 5], 1, 0, 1),
                    [lambda x, r: (x[0] + 5) % M]))
    out.append(Case("quad3", 2, 3, 1, 2,
                    compile_program([var(0) * var(1) - var(2), -var(0) + rand(0) * var(1) + 7], 3, 1, 2),
                    [lambda x, r: (x[0] * x[1] - x[2]) % M,
                     lambda x, r: (-x[0] + r[0] * x[1] + 7) % M], seed=b"quad3-seed!"))  # 11 bytes
    # declared degree 5 above the formal 4
    out.append(Case("deg5_w7", 5, 7, 2, 5,
                    compile_program([var(0) * var(1) * var(2) * var(3) - var(4),
                                     var(5) * var(6) - rand(0),
                                     var(0) - var(6) * 3,
                                     -(var(1) * var(1)) + rand(1) * var(2),
                                     var(3)], 7, 2, 5),
                    [lambda x, r: (x[0] * x[1] * x[2] * x[3] - x[4]) % M,
                     lambda x, r: (x[5] * x[6] - r[0]) % M,
                     lambda x, r: (x[0] - x[6] * 3) % M,
                     lambda x, r: (-(x[1] * x[1]) + r[1] * x[2]) % M,
                     lambda x, r: x[3] % M], seed=b"deg5"))
    out.append(Case("wide32", 9, 32, 0, 2, _wide32_wire(),
                    [lambda x, r: sum(x[i] * x[(i + 1) % 32] for i in range(32)) % M,
                     lambda x, r: (-(x[31] * x[0])) % M], seed=b"wide32w"))  # 7 bytes
    # 2^13 rows: more than one block, more than one row pair per thread
    out.append(Case("cubic4", 13, 4, 1, 3,
                    compile_program([var(0) * var(1) * var(2) - var(3),
                                     var(0) * var(0) + var(1) * var(1) - var(2) * var(2) * rand(0),
                                     var(0) + var(1) - var(3)], 4, 1, 3),
                    [lambda x, r: (x[0] * x[1] * x[2] - x[3]) % M,
                     lambda x, r: (x[0] * x[0] + x[1] * x[1] - x[2] * x[2] * r[0]) % M,
                     lambda x, r: (x[0] + x[1] - x[3]) % M], seed=b"cubic4-x"))
    return out


def all_programs():
    """(name, wire, width, randoms, callables) of every program the GPU tests run."""
    progs = [(c.name, c.wire, c.width, c.randoms, c.fns) for c in cases()]
    progs.append(("pythagorean", compile_program(pythagorean_exprs(), 4, 0, 2), 4, 0, PYTHAGOREAN_FNS))
    progs.append(("x0", compile_program([var(0)], 1, 0, 1), 1, 0, [lambda x, r: x[0] % M]))
    return progs
