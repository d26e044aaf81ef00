"""The sequential loop ms_build_extension_columns restates (include/ministark_hip_ext.h), on Python integers: the comparison of
tests/test_extension_columns.py, test_extension_prover.py and test_extension_mirror.py.  Fq3 arithmetic is oracle.pyref.fields'."""
import numpy as np

from oracle.pyref.fields import F252, FQ3, GL
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, STARK252_FP as F252F


class Pair:
    """a (base field -> extension field) pair: values are canonical ints, or 3-tuples for Fq3"""

    def __init__(self, base_field, ext_field):
        self.base_field, self.ext_field = base_field, ext_field
        self.bf = F252 if base_field == F252F else GL
        self.cubic = ext_field == FQ3F
        self.zero, self.one = ((0, 0, 0), (1, 0, 0)) if self.cubic else (0, 1)

    def embed(self, b):
        return (b, 0, 0) if self.cubic else b

    def add(self, x, y):
        return FQ3.add(x, y) if self.cubic else self.bf.add(x, y)

    def mul(self, x, y):
        return FQ3.mul(x, y) if self.cubic else self.bf.mul(x, y)

    def neg(self, x):
        return FQ3.neg(x) if self.cubic else self.bf.neg(x)

    def _limbs(self, v):
        m = self.bf.to_mont(v)
        return [(m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(self.bf.nlimbs)]

    def base_words(self, vals):
        return np.array([w for v in vals for w in self._limbs(v)], dtype=np.uint64)

    def ext_words(self, vals):
        if self.cubic:
            return np.array([GL.to_mont(c) for v in vals for c in v], dtype=np.uint64)
        return self.base_words(vals)

    def random_base(self, rng, n):
        return [int.from_bytes(rng.bytes(40), "little") % self.bf.p for _ in range(n)]

    def random_ext(self, rng, n):
        if self.cubic:
            return [tuple(self.random_base(rng, 3)) for _ in range(n)]
        return self.random_base(rng, n)


PAIRS = {"fp_fq3": Pair(FP, FQ3F), "fp_fp": Pair(FP, FP), "fp252_fp252": Pair(F252F, F252F)}


def reference(pair, base, challenges, columns):
    """base: lists of canonical ints (equally long); challenges: extension values; columns: ExtColumn records -> one list of extension
    values per column"""
    n = len(base[0])
    outs = []
    for c in columns:
        def value(terms, empty, i):
            if not terms:
                return empty
            acc = pair.zero
            for t in terms:
                sign, chal, col = t[0], t[1], t[2]
                off = t[3] if len(t) > 3 else 0
                v = pair.one if chal is None else challenges[chal]
                if col is not None:
                    v = pair.mul(v, pair.embed(base[col][(i + off) % n]))
                acc = pair.add(acc, v if sign > 0 else pair.neg(v))
            return acc
        state = challenges[c.init[1]] if isinstance(c.init, tuple) else (pair.one if c.init == 1 else pair.zero)
        out = []
        for i in range(n):
            if not c.inclusive:
                out.append(state)
            active = True if c.mask is None else (base[c.mask[1]][i] != 0) == (c.mask[0] == "nonzero")
            if active:
                state = pair.add(pair.mul(value(c.a_terms, pair.one, i), state), value(c.b_terms, pair.zero, i))
            if c.inclusive:
                out.append(state)
        outs.append(out)
    return outs
