"""The sequential loop ms_build_logup_columns restates (include/ministark_hip_logup.h), on Python integers: the comparison of
tests/test_logup_columns.py, test_logup_prover.py and test_logup_mirror.py.  The fields are tests/ext_ref.Pair's; inverses are
pow(x, -1, p) over the prime fields and, over Fq3, the adjugate over the norm -- the candidate is multiplied back with
oracle.pyref.fields.FQ3.mul and has to give one, so no formula is trusted -- with 0 -> 0, the library's convention."""
from oracle.pyref.fields import FQ3

from tests.ext_ref import PAIRS, Pair  # noqa: F401  (re-exported: the tests take both from here)


def inverse(pair, x):
    """x^-1 in the pair's extension field; inv(0) = 0"""
    if x == pair.zero:
        return pair.zero
    if not pair.cubic:
        return pow(x, -1, pair.bf.p)
    p = pair.bf.p
    a, b, c = x                                                # a + b X + c X^2,  X^3 = 2
    s = ((a * a - 2 * b * c) % p, (2 * c * c - a * b) % p, (b * b - a * c) % p)
    norm = FQ3.mul(x, s)
    assert norm[1] == 0 and norm[2] == 0 and norm[0] != 0
    inv = FQ3.mul_base(s, pow(norm[0], -1, p))
    assert FQ3.mul(x, inv) == FQ3.one()
    return inv


def value(pair, base, challenges, terms, i):
    """sum_t sign_t coef_t base[col_t][(i + off_t) mod n]"""
    n = len(base[0])
    acc = pair.zero
    for t in terms:
        sign, chal, col = t[0], t[1], t[2]
        off = t[3] if len(t) > 3 else 0
        v = pair.one if chal is None else challenges[chal]
        if col is not None:
            v = pair.mul(v, pair.embed(base[col][(i + off) % n]))
        acc = pair.add(acc, v if sign > 0 else pair.neg(v))
    return acc


def reference(pair, base, challenges, columns):
    """base: lists of canonical ints (equally long); challenges: extension values; columns: LogUpColumn records -> one list of extension
    values per column"""
    n = len(base[0])
    outs = []
    for c in columns:
        state = challenges[c.init[1]] if isinstance(c.init, tuple) else (pair.one if c.init == 1 else pair.zero)
        out = []
        for i in range(n):
            if not c.inclusive:
                out.append(state)
            active = True if c.mask is None else (base[c.mask[1]][i] != 0) == (c.mask[0] == "nonzero")
            if active:
                for num, den in c.fractions:
                    d = inverse(pair, value(pair, base, challenges, den, i))
                    state = pair.add(state, pair.mul(value(pair, base, challenges, num, i), d) if num else d)
            if c.inclusive:
                out.append(state)
        outs.append(out)
    return outs
