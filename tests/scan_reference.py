"""Plain-Python model of mlh_trace_scan (include/mlhip.h): exclusive running
sums and running products down columns of a row-major matrix of integers mod
M.  Nothing here is shared with the library.  Not a test module."""

M = 2 ** 128 - 45 * 2 ** 40 + 1


def combine(op, a, b):
    if op == "add":
        return (a + b) % M
    if op == "mul":
        return a * b % M
    raise ValueError(op)


def scan_matrix(matrix, width, scans):
    """matrix: height * width ints, row-major.  scans: [(op, src, dst, init)].
    -> (the matrix after the call, the totals).  Every scan reads its source
    column as the matrix stood at entry; z[0] = init, z[i + 1] = z[i] op t[i],
    column dst = z, total = z[height - 1] op t[height - 1]."""
    height = len(matrix) // width
    assert height * width == len(matrix) and height >= 1
    out, totals = list(matrix), []
    for op, src, dst, init in scans:
        z = init % M
        for i in range(height):
            out[i * width + dst] = z
            z = combine(op, z, matrix[i * width + src])
        totals.append(z)
    return out, totals
