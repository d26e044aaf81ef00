"""The three loops of include/ministark_hip_bitwise.h on Python integers: what tests/test_bitwise_columns.py,
test_bitwise_multiplicities.py and test_bitwise_prover.py compare the device against.  Columns are lists of canonical integers; a mask is
None, ("nonzero", m) or ("zero", m), as in ministark_amd.extension; an op is its code: 0 AND, 1 OR, 2 XOR."""
from tests.range_ref import LIMB_REPORT_FIELDS, RANGE_REPORT_FIELDS, active  # noqa: F401

AND, OR, XOR = 0, 1, 2


def apply(op, x, y):
    return x & y if op == AND else x | y if op == OR else x ^ y


def bitwise_columns(base, specs, n=None):
    """specs: objects with op, a, b, dst, width, mask.  -> (the base columns after the call, the report as a dict).  Rows from n on, and
    columns no spec writes, stay as they are."""
    n = len(base[0]) if n is None else n
    out = [list(c) for c in base]
    overflow = nactive = 0
    first = None
    for k, sp in enumerate(specs):
        W = 1 << sp.width
        for i in range(n):
            if not active(base, sp.mask, i):
                out[sp.dst][i] = 0
                continue
            va, vb = base[sp.a][i], base[sp.b][i]
            nactive += 1
            out[sp.dst][i] = apply(sp.op, va % W, vb % W)
            if va >= W or vb >= W:
                overflow += 1
                first = min(first, (k, i)) if first is not None else (k, i)
    return out, {"overflow": overflow, "first_overflow_spec": first[0] if first else 0, "first_overflow_row": first[1] if first else 0, "active": nactive}


def bitwise_table(bits, ops, n_t):
    """-> [top, tx, ty, tz], n_t integers each"""
    T, lm = len(ops) << (2 * bits), (1 << bits) - 1
    cols = [[], [], [], []]
    for j in range(n_t):
        r = min(j, T - 1)
        s, x, y = r >> (2 * bits), (r >> bits) & lm, r & lm
        for c, v in zip(cols, (ops[s], x, y, apply(ops[s], x, y))):
            c.append(v)
    return cols


def bitwise_multiplicities(base, bits, ops, sets, n_m, n=None):
    """sets: objects with op, a, b, c (None: no result column), nlimbs, mask.  -> (m as a list of n_m integers, the report as a dict)"""
    n = (len(base[0]) if base else 0) if n is None else n
    T, lm = len(ops) << (2 * bits), (1 << bits) - 1
    cnt = [0] * T
    missing = 0
    first = None
    for s, st in enumerate(sets):
        slot, W = list(ops).index(st.op), 1 << (st.nlimbs * bits)
        for i in range(n):
            if active(base, st.mask, i):
                va, vb = base[st.a][i], base[st.b][i]
                vc = base[st.c][i] if st.c is not None else apply(st.op, va, vb)
                if va >= W or vb >= W or vc != apply(st.op, va, vb):
                    missing += 1
                    first = min(first, (s, i)) if first is not None else (s, i)
                else:
                    for j in range(st.nlimbs):
                        cnt[(slot << (2 * bits)) + (((va >> (j * bits)) & lm) << bits) + ((vb >> (j * bits)) & lm)] += 1
    return cnt + [0] * (n_m - T), {"missing": missing, "first_missing_set": first[0] if first else 0, "first_missing_row": first[1] if first else 0,
                                   "duplicate_table_rows": 0}
