"""Plain-Python model of mlh_trace_lookup_tuple_counts (include/mlhip.h): the
multiplicity column of a lookup with tuple keys over a row-major list of ints.

key(j) = (matrix[j][T0], ..., matrix[j][Ta-1]) in the order of table_columns;
row j owns its key when no lower row has it.  value(i, l) is the same over
value tuple l of row i.  A pair (i, l) is enabled when there are no selectors,
selectors[l] is None, or matrix[i][selectors[l]] != 0.  The owner's count
element receives the number of enabled pairs whose value is its key, every
other row's zero; enabled pairs whose value is no key are counted, and the
lowest row with one is reported.  A disabled pair is neither."""


def lookup_tuple_counts(matrix, width, value_tuples, table_columns, count_column, selectors=None):
    """-> (the matrix afterwards, n_missing, first_missing_row or None)."""
    assert len(matrix) % width == 0
    h = len(matrix) // width
    table = tuple(table_columns)
    tuples = [tuple(t) for t in value_tuples]
    arity = len(table)
    assert 1 <= arity <= 8 and 1 <= len(tuples) <= 16 and arity * len(tuples) <= 32
    assert len(set(table)) == arity and all(0 <= c < width for c in table)
    assert 0 <= count_column < width and count_column not in table
    for t in tuples:
        assert len(t) == arity
        assert all(0 <= c < width and c not in table and c != count_column for c in t)
    sels = [None] * len(tuples) if selectors is None else list(selectors)
    assert len(sels) == len(tuples)
    assert all(s is None or (0 <= s < width and s != count_column) for s in sels)
    owner = {}
    for j in range(h):
        owner.setdefault(tuple(matrix[j * width + c] for c in table), j)
    counts = [0] * h
    n_missing, first = 0, None
    for i in range(h):
        for t, s in zip(tuples, sels):
            if s is not None and matrix[i * width + s] == 0:
                continue
            j = owner.get(tuple(matrix[i * width + c] for c in t))
            if j is None:
                n_missing += 1
                if first is None:
                    first = i
            else:
                counts[j] += 1
    out = list(matrix)
    out[count_column::width] = counts
    return out, n_missing, first
