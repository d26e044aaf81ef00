"""The loop ms_lookup_multiplicities restates (include/ministark_hip_lookup.h), on Python integers: the comparison of
tests/test_lookup_multiplicities.py, test_lookup_prover.py and test_lookup_mirror.py.  A base column is a list of integers and a key is the
tuple of a row's integers: for canonical input, one value is one Montgomery residue is one sequence of words, so equality of the integers
is the word-for-word comparison of the library."""


def active(base, t, i):
    """t: a LookupTuple (cols, mask)"""
    return True if t.mask is None else (base[t.mask[1]][i] != 0) == (t.mask[0] == "nonzero")


def key(base, t, i):
    return tuple(base[c][i] for c in t.cols)


def reference(base, table, lookups):
    """-> (cnt, report): cnt[j] the multiplicity of table row j as an integer, report a dict with the fields of ms_lookup_report"""
    n = len(base[0])
    first, dups = {}, 0
    for j in range(n):
        if active(base, table, j):
            k = key(base, table, j)
            if k in first:
                dups += 1
            else:
                first[k] = j
    cnt, missing, where = [0] * n, 0, None
    for s, t in enumerate(lookups):
        for i in range(n):
            if active(base, t, i):
                j = first.get(key(base, t, i))
                if j is None:
                    missing += 1
                    where = (s, i) if where is None else min(where, (s, i))
                else:
                    cnt[j] += 1
    s, i = where or (0, 0)
    return cnt, {"missing": missing, "first_missing_set": s, "first_missing_row": i, "duplicate_table_rows": dups}
