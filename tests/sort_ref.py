"""The loop ms_sort_rows restates (include/ministark_hip_sort.h), on Python integers: the comparison of tests/test_sort_rows.py,
test_sort_prover.py and test_sort_mirror.py.  A base column is a list of canonical integers; Python's `sorted` is stable, which is the
order the library promises for rows of equal keys."""


def active(base, key, i):
    """key: a SortKey (cols, mask)"""
    return True if key.mask is None else (base[key.mask[1]][i] != 0) == (key.mask[0] == "nonzero")


def reference(base, key, nbytes, n=None):
    """-> (perm, report): perm the list of row indices, report a dict with the fields of ms_sort_report.  nbytes: the bytes of a canonical
    element (8 or 32); n: the rows to sort (default: all)."""
    n = len(base[0]) if n is None else n
    act = [i for i in range(n) if active(base, key, i)]
    ina = [i for i in range(n) if not active(base, key, i)]
    perm = sorted(act, key=lambda i: tuple(base[c][i] for c in key.cols)) + ina
    varying = 0
    for c in key.cols:
        vals = {base[c][i] for i in act}
        if len(vals) > 1:
            first = next(iter(vals))
            diff = 0
            for v in vals:
                diff |= v ^ first
            varying += sum(1 for b in range(nbytes) if (diff >> (8 * b)) & 0xFF)
    return perm, {"active": len(act), "varying_bytes": varying}


def permuted(col, index, n_src=None):
    """col[index[i]], zero where index[i] is no row"""
    n_src = len(col) if n_src is None else n_src
    return [col[j] if j < n_src else 0 for j in index]
