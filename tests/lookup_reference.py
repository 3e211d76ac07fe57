"""Plain-Python model of mlh_trace_lookup_counts (include/mlhip.h): the
multiplicity column of a lookup over a row-major list of ints.

key(j) = matrix[j][T]; row j owns its key when no lower row has it.  The owner's
count element receives the number of (row, value column) pairs whose value is
that key, every other row's zero; pairs whose value is no table entry are
counted, and the lowest row with one is reported."""


def lookup_counts(matrix, width, value_columns, table_column, count_column):
    """-> (the matrix afterwards, n_missing, first_missing_row or None)."""
    assert len(matrix) % width == 0
    h = len(matrix) // width
    cols = sorted(set(value_columns))
    assert cols and all(0 <= c < width for c in cols)
    assert 0 <= table_column < width and 0 <= count_column < width
    assert table_column != count_column
    assert table_column not in cols and count_column not in cols
    owner = {}
    for j in range(h):
        owner.setdefault(matrix[j * width + table_column], j)
    counts = [0] * h
    n_missing, first = 0, None
    for i in range(h):
        for c in cols:
            j = owner.get(matrix[i * width + c])
            if j is None:
                n_missing += 1
                if first is None:
                    first = i
            else:
                counts[j] += 1
    out = list(matrix)
    out[count_column::width] = counts
    return out, n_missing, first
