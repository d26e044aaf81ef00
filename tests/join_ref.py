"""The loop ms_join_rows restates (include/ministark_hip_join.h), on Python integers: the comparison of tests/test_join_rows.py,
test_join_prover.py and test_join_mirror.py.  It uses nothing of the library.  A column is a list of integers and a key is the tuple of a
row's integers: for canonical input, one value is one Montgomery residue is one sequence of words, so equality of the integers is the
word-for-word comparison of the library.  A key record is anything with `.cols` and `.mask` (None, ("nonzero", m) or ("zero", m))."""

NONE = 0xFFFFFFFF
REPORT_FIELDS = ("matched", "missing", "first_missing_set", "first_missing_row", "duplicate_table_rows", "table_active")


def active(cols, t, i):
    return True if t.mask is None else (cols[t.mask[1]][i] != 0) == (t.mask[0] == "nonzero")


def key(cols, t, i):
    return tuple(cols[c][i] for c in t.cols)


def first_rows(table, table_key, n_table):
    """-> (first, duplicates, active rows)"""
    first, dups, tact = {}, 0, 0
    for j in range(n_table):
        if active(table, table_key, j):
            tact += 1
            k = key(table, table_key, j)
            if k in first:
                dups += 1
            else:
                first[k] = j
    return first, dups, tact


def reference(table, table_key, base, keys, n_table=None, n=None):
    """-> (match, report): match[s][i] a table row or NONE, report a dict with the fields of ms_join_report.
    n_table, n: the row counts, when a side has no column to take them from"""
    n_table = len(table[0]) if n_table is None else n_table
    n = len(base[0]) if n is None else n
    first, dups, tact = first_rows(table, table_key, n_table)
    match, matched, missing, where = [], 0, 0, None
    for s, t in enumerate(keys):
        out = [NONE] * n
        for i in range(n):
            if active(base, t, i):
                j = first.get(key(base, t, i))
                if j is None:
                    missing += 1
                    where = (s, i) if where is None else min(where, (s, i))
                else:
                    out[i] = j
                    matched += 1
        match.append(out)
    s, i = where or (0, 0)
    return match, {"matched": matched, "missing": missing, "first_missing_set": s, "first_missing_row": i, "duplicate_table_rows": dups, "table_active": tact}
