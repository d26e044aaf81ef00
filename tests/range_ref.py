"""The two loops of include/ministark_hip_range.h on Python integers: what tests/test_limb_decompose.py, test_range_multiplicities.py
and test_range_prover.py compare the device against.  Columns are lists of canonical integers; a mask is None, ("nonzero", m) or
("zero", m), as in ministark_amd.extension."""

LIMB_REPORT_FIELDS = ("overflow", "first_overflow_spec", "first_overflow_row", "active")
RANGE_REPORT_FIELDS = ("missing", "first_missing_set", "first_missing_row", "duplicate_table_rows")


def active(base, mask, i):
    if mask is None:
        return True
    kind, m = mask
    return (base[m][i] != 0) == (kind == "nonzero")


def limb_decompose(base, specs, n=None):
    """specs: objects with src, dst0, nlimbs, bits, mask.  -> (the base columns after the call, the report as a dict).  Rows from n on, and
    columns no spec writes, stay as they are."""
    n = len(base[0]) if n is None else n
    out = [list(c) for c in base]
    overflow = nactive = 0
    first = None
    for k, sp in enumerate(specs):
        for i in range(n):
            if not active(base, sp.mask, i):
                for j in range(sp.nlimbs):
                    out[sp.dst0 + j][i] = 0
                continue
            v = base[sp.src][i]
            nactive += 1
            for j in range(sp.nlimbs):
                out[sp.dst0 + j][i] = (v >> (j * sp.bits)) & ((1 << sp.bits) - 1)
            if v >> (sp.nlimbs * sp.bits):
                overflow += 1
                first = min(first, (k, i)) if first is not None else (k, i)
    return out, {"overflow": overflow, "first_overflow_spec": first[0] if first else 0, "first_overflow_row": first[1] if first else 0, "active": nactive}


def range_multiplicities(base, bits, sets, n_m, n=None):
    """sets: objects with col, mask.  -> (m as a list of n_m integers, the report as a dict)"""
    n = (len(base[0]) if base else 0) if n is None else n
    cnt = [0] * (1 << bits)
    missing = 0
    first = None
    for s, st in enumerate(sets):
        col = base[st.col]
        for i in range(n):
            if active(base, st.mask, i):
                v = col[i]
                if v < (1 << bits):
                    cnt[v] += 1
                else:
                    missing += 1
                    first = min(first, (s, i)) if first is not None else (s, i)
    return cnt + [0] * (n_m - (1 << bits)), {"missing": missing, "first_missing_set": first[0] if first else 0, "first_missing_row": first[1] if first else 0,
                                           "duplicate_table_rows": 0}
