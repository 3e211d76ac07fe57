"""Plain-Python model of the witness check (mlh_trace_check /
mlh_trace_check_public), for tests/test_trace_check_*.py.  No libmlhip
arithmetic: the constraints are callables f(var, rand) -> int over the W + K
wide row of the extension, which tests/shifted_reference.extend builds by plain
indexing, and the public strip is tests/public_reference.strip.

A result is the tuple (bad_rows, first_bad_row, first_bad_constraint, counts,
first_rows) with None where the library reports "none": the fields of
multilinear_amd.constraint_system.CheckResult, in that order.
"""
import public_reference as PUB
import shifted_reference as SR

M = SR.M


def _result(fails, n, rows):
    """fails(i) -> the failing constraints of row i, ascending."""
    counts, firsts = [0] * n, [None] * n
    bad, first_row, first_c = 0, None, None
    for i in range(rows):
        f = fails(i)
        if f:
            bad += 1
            if first_row is None:
                first_row, first_c = i, f[0]
        for c in f:
            counts[c] += 1
            if firsts[c] is None:
                firsts[c] = i
    return (bad, first_row, first_c, counts, firsts)


def check(fns, matrix, width, shifts, log_height, randoms=()):
    """Every f of fns on every row extended with the next row's source
    columns, cyclically; a constraint fails where its value is not 0 mod M."""
    H, Wx = 1 << log_height, width + len(shifts)
    E = SR.extend(matrix, width, list(shifts), H)
    rnd = list(randoms)

    def fails(i):
        row = E[i * Wx:(i + 1) * Wx]
        return [c for c, f in enumerate(fns) if f(row, rnd) % M != 0]

    return _result(fails, len(fns), H)


def check_public(matrix, width, descs, log_height):
    """The last len(descs) columns against the strip of the description."""
    H, F = 1 << log_height, len(descs)
    st = PUB.strip(descs, H)

    def fails(i):
        return [j for j in range(F) if matrix[i * width + width - F + j] != st[i * F + j]]

    return _result(fails, F, H)


def as_tuple(res):
    """A CheckResult as the model's tuple."""
    return (res.bad_rows, res.first_bad_row, res.first_bad_constraint, list(res.counts),
            list(res.first_rows))
