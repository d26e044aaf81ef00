"""The loops ms_gap_plan and ms_gap_fill restate (include/ministark_hip_gaps.h), on Python integers: the comparison of
tests/test_gap_rows.py, test_gap_prover.py and test_gap_mirror.py.  A base column is a list of canonical integers; `spec` is a GapSpec
(group, counter, mask), `perm` a list of row indices or None."""

CAP = 1 << 32
NONE_UNORDERED = (1 << 64) - 1


def plan(base, spec, perm=None, n=None, n_src=None):
    """-> (start, report): start the n + 1 prefix sums, report a dict with the fields of ms_gap_report"""
    n_src = len(base[0]) if n_src is None else n_src
    held = n_src if perm is None else len(perm)
    n = held if n is None else n
    row = (lambda j: j) if perm is None else (lambda j: perm[j])

    def act(j):
        r = row(j)
        if r >= n_src:
            return False
        return True if spec.mask is None else (base[spec.mask[1]][r] != 0) == (spec.mask[0] == "nonzero")

    rep = {"active": 0, "rows_out": 0, "gaps": 0, "max_gap": 0, "unordered": 0, "first_unordered": NONE_UNORDERED, "saturated": 0}
    start = [0]
    for j in range(n):
        cnt = 0
        if act(j):
            gap = 0
            if spec.counter is not None and j + 1 < n and act(j + 1) and all(base[g][row(j)] == base[g][row(j + 1)] for g in spec.group):
                d = base[spec.counter][row(j + 1)] - base[spec.counter][row(j)]
                if d >= 2:
                    gap = min(d - 1, CAP)
                    rep["saturated"] += d - 1 > CAP
                elif d <= 0:
                    rep["unordered"] += 1
                    rep["first_unordered"] = min(rep["first_unordered"], j)
            cnt = 1 + gap
            rep["active"] += 1
            rep["gaps"] += gap > 0
            rep["max_gap"] = max(rep["max_gap"], gap)
        start.append(start[-1] + cnt)
    rep["rows_out"] = start[-1]
    return start, rep


def fill(base, start, columns, n_out, p, perm=None, rows=None):
    """-> the len(columns) filled columns as lists of canonical integers.  columns: (kind, src) with kind "copy", "zero", "counter", "flag";
    p: the modulus; rows: the output rows to compute (default: range(n_out))"""
    import bisect
    n, rows_out = len(start) - 1, start[-1]
    out = [[] for _ in columns]
    for j in (range(n_out) if rows is None else rows):
        if rows_out == 0:
            for c, (kind, _) in enumerate(columns):
                out[c].append(1 if kind == "flag" else 0)
            continue
        jj = min(j, rows_out - 1)
        s = bisect.bisect_right(start, jj, 0, n) - 1                 # the largest position in [0, n) with start[s] <= jj
        k = j - start[s]
        r = s if perm is None else perm[s]
        for c, (kind, src) in enumerate(columns):
            if kind == "flag":
                out[c].append(0 if k == 0 else 1)
            elif kind == "copy":
                out[c].append(base[src][r])
            elif kind == "zero":
                out[c].append(base[src][r] if k == 0 else 0)
            else:
                out[c].append((base[src][r] + k) % p)
    return out
