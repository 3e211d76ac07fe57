"""Plain-Python model of mlh_trace_sort (include/mlhip.h): sorted copies of
columns of a row-major matrix of integers below 2^128, in stable ascending
order of up to 4 key columns compared as unsigned integers.  Nothing here is
shared with the library.  Not a test module."""

M = 2 ** 128 - 45 * 2 ** 40 + 1


def sort_matrix(matrix, width, keys, copies, perm_column=None):
    """matrix: height * width ints, row-major.  keys: the key columns, the most
    significant first.  copies: [(src, dst)].  -> (the matrix after the call,
    pi): pi(r) is the row of the r-th smallest key tuple, equal tuples in row
    order; column dst of row r = column src of row pi(r) as the matrix stood at
    entry, column perm_column of row r = pi(r)."""
    height = len(matrix) // width
    assert height * width == len(matrix) and height >= 1
    pi = sorted(range(height),
                key=lambda i: (tuple(int(matrix[i * width + k]) for k in keys), i))
    out = list(matrix)
    for r, i in enumerate(pi):
        for src, dst in copies:
            out[r * width + dst] = matrix[i * width + src]
        if perm_column is not None:
            out[r * width + perm_column] = i
    return out, pi
