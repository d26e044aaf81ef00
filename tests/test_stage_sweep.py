"""Sweep of the element-wise stages through the C ABI (ms_binary, ms_binary_const, ms_mul_pow, ms_unary, ms_convert, ms_fill,
ms_sum_columns), where `n` is free: every kernel template that csrc/ms_stage.cpp can launch, at ragged and tiny lengths, at the
batch-inverse tile edges, past the grid-stride cap of stream_grid (2^20 words), with every rotation and exponent edge, in
place and into another buffer.  Every output word is compared, bit-exact; every input a call must not touch is compared too,
and every buffer carries guard words behind its last element.

References: Goldilocks (Fp, Fq3, Fq3 x Fp) -- oracle.cref, itself pinned here against the big integers of oracle.pyref.fields.
The 252-bit field -- Python integers on the Montgomery words (R = 2^256): helpers in `class M252`.

The second half checks the aliasing rules of include/ministark_hip.h: a refused shape returns MS_ERR_INVALID with "overlap" in
ms_last_error() and leaves the destination as it was; the allowed shapes give the oracle's words."""
import collections
import ctypes

import numpy as np
import pytest

from oracle import cref
from oracle.pyref import fields as PF
from tests import backends
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as F252, GpuVec

P = cref.GL_P
P252 = PF.F252_P
V = {FP: 1, FQ3: 3, F252: 4}
FNAME = {FP: "fp", FQ3: "fq3", F252: "f252"}
ADD, MUL = 0, 1
NEG, INV, EXP = 0, 1, 2
MS_OK, MS_ERR_INVALID, MS_ERR_UNSUPPORTED = 0, -1, -2
LONG_MAX, LONG_MIN = (1 << 63) - 1, -(1 << 63)
CAP = 1 << 20                       # stream_grid: 4096 workgroups of 256 lanes; one more word and a lane takes a second element
PAIRS = [(FP, FP), (FQ3, FQ3), (FQ3, FP), (F252, F252)]
REFUSED_PAIRS = [(FP, FQ3), (F252, FP), (FQ3, F252)]
EXPONENTS = [0, 1, 2, 3, 1 << 31, (1 << 32) - 1]
ONE = {FP: np.array([0xFFFFFFFF], dtype=np.uint64), FQ3: np.array([0xFFFFFFFF, 0, 0], dtype=np.uint64),
       F252: np.array(cref.F252_ONE_MONT, dtype=np.uint64)}


def shifts_of(n):
    return [0, 1, -1, n - 1, n, -n, n + 1, -(n + 1), 2 * n + 3, (1 << 62) + 5, -((1 << 62) + 5), LONG_MAX, LONG_MIN]


# ------------------------------------------------------------------------------------------------------------------
# values
# ------------------------------------------------------------------------------------------------------------------
# the carry-edge words of tests/test_ntt_parity.py::_adversarial
GL_EDGE = np.array([0, 1, P - 1, P - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - (1 << 32), (1 << 63), (1 << 63) - 1,
                    0xFFFFFFFE00000001, 0xFFFFFFFEFFFFFFFF, 0x00000000FFFFFFFE, 0xFFFFFFFF00000000], dtype=np.uint64)


def gl_values(n, v, seed):
    """uniform words with the edge words sprinkled in; for Fq3 also whole elements (p-1, p-1, p-1) and (p-1, 0, p-1): Fq3T::mul adds
    components before it multiplies.  From two elements on, the last one is zero."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, P, size=n * v, dtype=np.uint64)
    m = rng.random(n * v) < 0.3
    a[m] = GL_EDGE[rng.integers(0, GL_EDGE.size, size=int(m.sum()))]
    a = a.reshape(n, v)
    if v == 3:
        k = rng.random(n)
        a[k < 0.06] = P - 1
        a[(k >= 0.06) & (k < 0.12)] = np.array([P - 1, 0, P - 1], dtype=np.uint64)
    if n >= 2:
        a[n - 1] = 0
    return np.ascontiguousarray(a.reshape(-1))


def _pool252():
    """the edge list and the digit-pattern generator of tests/test_fp252_parity.py::test_mul_edge_values_252 (nine 28-bit digits)."""
    rng = np.random.default_rng(11)
    M = (1 << 28) - 1
    edge = [0, 1, 2, P252 - 1, P252 - 2, P252 - (1 << 28), (1 << 28) - 1, 1 << 28, (1 << 252) - 1 - (1 << 200), (1 << 251), (1 << 251) + 17 * (1 << 192),
            sum(M << (28 * k) for k in range(0, 9, 2)), sum(M << (28 * k) for k in range(1, 9, 2)), (1 << 224) - 1, 1 << 224, (1 << 192) * 17, P252 >> 1]
    digits = []
    for _ in range(256):
        x = 0
        for k in range(9):
            x |= int(rng.choice([0, M, 1, M - 1, int(rng.integers(0, M + 1))])) << (28 * k)
        digits.append(x)
    return M252.words([x % P252 for x in edge]).reshape(-1, 4), M252.words([x % P252 for x in digits]).reshape(-1, 4)


class M252:
    """The 252-bit field on Python integers.  Device words are Montgomery residues w(x) = x R mod p, R = 2^256."""
    R = (1 << 256) % P252
    R2 = R * R % P252
    RINV = pow(R, -1, P252)
    _pool = None

    @staticmethod
    def ints(words):
        b = np.ascontiguousarray(words, dtype=np.uint64).tobytes()
        return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]

    @staticmethod
    def words(ints):
        return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in ints), dtype=np.uint64).copy()

    @classmethod
    def values(cls, n, seed):
        """canonical words: uniform below 2^251, the edge list (15 %) and digit patterns (20 %); the last element is zero from n = 2."""
        if cls._pool is None:
            cls._pool = _pool252()
        edge, digits = cls._pool
        rng = np.random.default_rng(seed)
        a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 59) - 1)
        k = rng.random(n)
        m = k < 0.15
        a[m] = edge[rng.integers(0, len(edge), size=int(m.sum()))]
        m = (k >= 0.15) & (k < 0.35)
        a[m] = digits[rng.integers(0, len(digits), size=int(m.sum()))]
        if n >= 2:
            a[n - 1] = 0
        return np.ascontiguousarray(a.reshape(-1))

    @staticmethod
    def add(a, b):
        return (a + b) % P252

    @staticmethod
    def neg(a):
        return (-a) % P252

    @classmethod
    def mul(cls, a, b):                       # w(x) w(y) R^-1 = w(x y)
        return a * b * cls.RINV % P252

    @classmethod
    def pow_factor(cls, e):
        """w(x^e) = w(x)^e R^(1-e): the factor that takes the R powers out (e >= 1)."""
        return pow(cls.RINV, e - 1, P252)

    @classmethod
    def pow(cls, a, e, factor=None):
        if e == 0:
            return cls.R                      # x^0 = 1, 0^0 included
        return pow(a, e, P252) * (cls.pow_factor(e) if factor is None else factor) % P252

    @classmethod
    def inv(cls, a):                          # w(x^-1) = w(x)^-1 R^2; 0 -> 0
        return 0 if a == 0 else pow(a, -1, P252) * cls.R2 % P252


def values(field, n, seed):
    return M252.values(n, seed) if field == F252 else gl_values(n, V[field], seed)


def rot(xs, shift):
    n = len(xs)
    s = shift % n
    return xs[s:] + xs[:s]


# ------------------------------------------------------------------------------------------------------------------
# references: words in, words out
# ------------------------------------------------------------------------------------------------------------------
def ref_binary(op, lf, rf, a, b, shift):
    if lf != F252:
        return cref.binary(op, V[lf], V[rf], a, b, shift)
    f = M252.add if op == ADD else M252.mul
    return M252.words([f(x, y) for x, y in zip(M252.ints(a), rot(M252.ints(b), shift))])


def ref_const(op, lf, rf, a, c):
    if lf != F252:
        return cref.binary_const(op, V[lf], V[rf], a, c)
    k = M252.ints(c)[0]
    return M252.words([(x + k) % P252 for x in M252.ints(a)] if op == ADD else [M252.mul(x, k) for x in M252.ints(a)])


def ref_mul_pow(lf, rf, a, b, e, shift):
    if lf != F252:
        return cref.mul_pow(V[lf], V[rf], a, b, e, shift)
    k = M252.pow_factor(e) if e else None
    return M252.words([M252.mul(x, M252.pow(y, e, k)) for x, y in zip(M252.ints(a), rot(M252.ints(b), shift))])


def ref_unary(op, f, a, e):
    if f != F252:
        return cref.unary(op, V[f], a, e)
    xs = M252.ints(a)
    if op == NEG:
        return M252.words([M252.neg(x) for x in xs])
    if op == INV:
        return M252.words([M252.inv(x) for x in xs])
    k = M252.pow_factor(e) if e else None
    return M252.words([M252.pow(x, e, k) for x in xs])


def check_inverse_252(src, got):
    """complete check by the product: w(a) w(a^-1) = R^2 (mod p) for a != 0, 0 -> 0, every word canonical (a word + p also fits 256 bits)."""
    xs, ys = M252.ints(src), M252.ints(got)
    R2 = M252.R2
    bad = [i for i, (x, y) in enumerate(zip(xs, ys)) if y >= P252 or (y != 0 if x == 0 else x * y % P252 != R2)]
    assert not bad, f"{len(bad)} wrong inverses, first at element {bad[0]}"


# ------------------------------------------------------------------------------------------------------------------
# device buffers with guard words behind the last element
# ------------------------------------------------------------------------------------------------------------------
GUARD = np.array([0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A] * 8, dtype=np.uint64)


class Buf:
    def __init__(self, pl, words):
        self.nw = int(words.size)
        self.vec = GpuVec.from_numpy(pl, np.concatenate([np.asarray(words, dtype=np.uint64), GUARD]), FP)
        self.ptr = self.vec.ptr

    @classmethod
    def junk(cls, pl, nwords):
        return cls(pl, np.full(nwords, 0xDEADBEEFDEADBEEF, dtype=np.uint64))

    def read(self):
        a = self.vec.to_numpy()
        assert np.array_equal(a[self.nw:], GUARD), "words behind the last element were written"
        return a[:self.nw]


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {bad.size} of {want.size} words differ, first at word {int(bad[0])}: "
                             f"got {int(got[bad[0]]):#x}, want {int(want[bad[0]]):#x}")


# ------------------------------------------------------------------------------------------------------------------
# the dispatch of csrc/ms_stage.cpp, restated by hand: which kernel template a call launches, and over how many words per element
# ------------------------------------------------------------------------------------------------------------------
def template_of(entry, op, lf, rf, n):
    vl, vr = V[lf], V[rf]
    T = {1: "FpT", 3: "Fq3T", 4: "Fp252T"}
    if entry == "binary":
        if vl == 3 and vr == 3 and op == ADD:
            return "k_binary<FpT,FpT,0> over 3n words (Fq3 + Fq3)"
        return f"k_binary<{T[vl]},{T[vr]},{op}>"
    if entry == "const":
        if vl == 3 and vr == 1 and op == MUL:
            return "k_binary_const<FpT,FpT,1> over 3n words (Fq3 * Fp const)"
        return f"k_binary_const<{T[vl]},{T[vr]},{op}>"
    if entry == "mul_pow":
        return f"k_mul_pow<{T[vl]},{T[vr]}>"
    if entry == "unary":
        if op == INV and n >= 4096:
            return f"k_batch_inverse<{T[vl]},{16 if vl == 1 else 8}>"
        if vl == 3 and op == NEG:
            return "k_unary<FpT,0> over 3n words (-Fq3)"
        return f"k_unary<{T[vl]},{op}>"
    if entry == "convert":
        return "k_convert_fp_fq3" if vl != vr else f"hipMemcpyAsync copy route ({FNAME[lf]})"
    if entry == "fill":
        return f"k_fill V={vl}"
    if entry == "sum":
        return "k_sum_columns252" if vl == 4 else f"k_sum_columns V={vl}"
    raise ValueError(entry)


def launch_words(entry, op, lf, rf):
    """words per element that the launch counts its lanes over (1: one lane per element)."""
    vl, vr = V[lf], V[rf]
    if entry == "binary" and vl == 3 and vr == 3 and op == ADD:
        return 3
    if entry == "const" and vl == 3 and vr == 1 and op == MUL:
        return 3
    if entry == "unary" and vl == 3 and op == NEG:
        return 3
    if entry == "fill" or (entry == "sum" and vl == 3):
        return vl
    return 1


Case = collections.namedtuple("Case", "entry op lf rf n shift e extra long kinds")
SMALL = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
OPNAME = {"binary": {ADD: "add", MUL: "mul"}, "const": {ADD: "add", MUL: "mul"}, "unary": {NEG: "neg", INV: "inv", EXP: "exp"}}


def lengths_of(entry, op, lf, rf):
    k = 256 * (16 if V[lf] == 1 else 8)                   # the batch-inverse tile: 16 elements per lane over Fp, 8 over Fq3 / Fp252
    tiles = [k * j + r for j in (1, 3) for r in (0, 1, 255)]
    w = launch_words(entry, op, lf, rf)
    longs = [CAP, CAP + 1, CAP + (1 << 18) + 13] if w == 1 else [-(-CAP // w) - 1, -(-CAP // w) + 1, (1 << 19) + 77]
    return SMALL + tiles, longs


def _forms():
    out = []
    for op in (ADD, MUL):
        out += [("binary", op, lf, rf) for lf, rf in PAIRS]
    for op in (ADD, MUL):
        out += [("const", op, lf, rf) for lf, rf in PAIRS]
    out += [("mul_pow", None, lf, rf) for lf, rf in PAIRS]
    out += [("unary", op, f, f) for op in (NEG, INV, EXP) for f in (FP, FQ3, F252)]
    out += [("convert", None, FQ3, FP)] + [("convert", None, f, f) for f in (FP, FQ3, F252)]
    out += [("fill", None, f, f) for f in (FP, FQ3, F252)]
    out += [("sum", None, f, f) for f in (FP, FQ3, F252)]
    return out


def _cases():
    """Pairwise, not a product: the lengths of a form (11 small, 6 tile edges, 3 long) are walked once, and the shifts (13), exponents (6),
    column counts (4) and sum aliasings (3) cycle along them -- 20 lengths per form, so every value of every axis meets every template."""
    cases = []
    for fi, (entry, op, lf, rf) in enumerate(_forms()):
        short, longs = lengths_of(entry, op, lf, rf)
        for li, n in enumerate(short + longs):
            is_long = li >= len(short)
            shift = shifts_of(n)[(li + fi) % 13] if entry in ("binary", "mul_pow") else None
            e = None
            if entry == "mul_pow" or (entry == "unary" and op == EXP):
                # the big exponents over Fp252 stay below 2^13 elements (one Python pow per element); every exponent still meets every template
                e = EXPONENTS[(li + fi) % 6] if (lf != F252 or n < (1 << 13)) else EXPONENTS[(li + fi) % 4]
            extra = ((1, 2, 127, 128)[(li + fi) % 4], ("none", "first", "last")[li % 3]) if entry == "sum" else None
            kinds = ["emu", "hip"]
            if is_long:
                # simulator: one long length per template (past the cap), cheap operations only: add, mul, neg, fill, convert, copy, sum, batch inverse
                cheap = entry in ("binary", "const", "convert", "fill", "sum") or (entry == "unary" and op in (NEG, INV))
                if not cheap or (li - len(short)) != (2 if launch_words(entry, op, lf, rf) > 1 else 1 + fi % 2):
                    kinds = ["hip"]
            cases.append(Case(entry, op, lf, rf, n, shift, e, extra, is_long, tuple(kinds)))
    return cases


def case_id(c):
    s = c.entry + ("-" + OPNAME[c.entry][c.op] if c.entry in OPNAME else "") + "-" + FNAME[c.lf] + ("x" + FNAME[c.rf] if c.rf != c.lf or c.entry in ("binary", "const", "mul_pow") else "")
    s += f"-n{c.n}"
    if c.shift is not None:
        s += f"-sh{c.shift}"
    if c.e is not None:
        s += f"-e{c.e}"
    if c.extra is not None:
        s += f"-cols{c.extra[0]}-dst_{c.extra[1]}"
    return s


CASES = _cases()
SWEEP = [pytest.param(kind, c, id=kind + "-" + case_id(c), marks=[pytest.mark.gpu] if kind == "hip" else [])
         for c in CASES for kind in c.kinds]


# ------------------------------------------------------------------------------------------------------------------
# one case
# ------------------------------------------------------------------------------------------------------------------
def zero_power(f, e):
    return ONE[f] if e == 0 else np.zeros(V[f], dtype=np.uint64)


def run_case(pl, c, seed):
    L, h, n = pl.lib, pl.handle, c.n
    vl, vr = V[c.lf], V[c.rf]
    if c.entry in ("binary", "mul_pow"):
        a, b = values(c.lf, n, seed), values(c.rf, n, seed + 1)
        if c.entry == "binary":
            want = ref_binary(c.op, c.lf, c.rf, a, b, c.shift)
            call = lambda d, l, r, sh=c.shift: L.ms_binary(h, c.op, c.lf, c.rf, n, d, l, r, sh)
        else:
            want = ref_mul_pow(c.lf, c.rf, a, b, c.e, c.shift)
            call = lambda d, l, r, sh=c.shift: L.ms_mul_pow(h, c.lf, c.rf, n, d, l, r, c.e, sh)
            if n >= 2:               # rhs[n-1] = 0 meets lhs[i]: 0^0 = 1 leaves lhs[i], 0^e = 0 clears it
                i = (n - 1 - c.shift) % n
                same(want[i * vl:(i + 1) * vl], a[i * vl:(i + 1) * vl] if c.e == 0 else np.zeros(vl, dtype=np.uint64), "0^e in the reference")
        A, B, D = Buf(pl, a), Buf(pl, b), Buf.junk(pl, n * vl)
        assert call(D.ptr, A.ptr, B.ptr) == MS_OK
        same(D.read(), want, "Into"); same(A.read(), a, "lhs of the Into form"); same(B.read(), b, "rhs of the Into form")
        assert call(A.ptr, A.ptr, B.ptr) == MS_OK
        same(A.read(), want, "Assign"); same(B.read(), b, "rhs of the Assign form")
        if c.lf == c.rf and c.shift % n == 0:      # the allowed extra: dst == lhs == rhs, every lane on its own index
            S = Buf(pl, a)
            assert call(S.ptr, S.ptr, S.ptr) == MS_OK
            same(S.read(), ref_binary(c.op, c.lf, c.rf, a, a, 0) if c.entry == "binary" else ref_mul_pow(c.lf, c.rf, a, a, c.e, 0), "dst == lhs == rhs")
    elif c.entry == "const":
        a, k = values(c.lf, n, seed), values(c.rf, 1, seed + 1)
        want = ref_const(c.op, c.lf, c.rf, a, k)
        A, D = Buf(pl, a), Buf.junk(pl, n * vl)
        assert L.ms_binary_const(h, c.op, c.lf, c.rf, n, D.ptr, A.ptr, k.ctypes.data) == MS_OK
        same(D.read(), want, "IntoConst"); same(A.read(), a, "lhs of the IntoConst form")
        assert L.ms_binary_const(h, c.op, c.lf, c.rf, n, A.ptr, A.ptr, k.ctypes.data) == MS_OK
        same(A.read(), want, "AssignConst")
    elif c.entry == "unary":
        a = values(c.lf, n, seed)
        e = c.e or 0
        by_product = c.op == INV and c.lf == F252
        want = ref_unary(c.op, c.lf, a, e) if not (by_product and n >= (1 << 13)) else None
        A, D = Buf(pl, a), Buf.junk(pl, n * vl)
        for dst, what in ((D, "Into"), (A, "InPlace")):
            assert L.ms_unary(h, c.op, c.lf, n, dst.ptr, A.ptr, e) == MS_OK
            got = dst.read()
            if want is not None:
                same(got, want, what)
            if by_product:
                check_inverse_252(a, got)
            if c.op == EXP and n >= 2:
                same(got[(n - 1) * vl:], zero_power(c.lf, e), "0^e")
            if c.op == INV and n >= 2:
                assert not got[(n - 1) * vl:].any(), "0^-1 = 0"
            if dst is D:
                same(A.read(), a, "src of the Into form")
    elif c.entry == "convert":
        a = values(c.rf, n, seed)
        A, D = Buf(pl, a), Buf.junk(pl, n * vl)
        assert L.ms_convert(h, c.lf, c.rf, n, D.ptr, A.ptr) == MS_OK
        if vl == vr:
            want = a
        else:
            want = np.zeros((n, 3), dtype=np.uint64); want[:, 0] = a; want = want.reshape(-1)
        same(D.read(), want, "ConvertInto"); same(A.read(), a, "src")
        if vl == vr:                                 # the same buffer: a no-op
            assert L.ms_convert(h, c.lf, c.rf, n, A.ptr, A.ptr) == MS_OK
            same(A.read(), a, "convert onto itself")
    elif c.entry == "fill":
        k = values(c.lf, 1, seed)
        D = Buf.junk(pl, n * vl)
        assert L.ms_fill(h, c.lf, n, D.ptr, k.ctypes.data) == MS_OK
        same(D.read(), np.tile(k, n), "FillBuff")
    elif c.entry == "sum":
        ncols, alias = c.extra
        distinct = [values(c.lf, n, seed + i) for i in range(min(ncols, 3))]
        idx = [0] + [1 + (j % 2) for j in range(ncols - 1)] if ncols > 1 else [0]      # columns may alias each other: they are only read
        bufs = [Buf(pl, d) for d in distinct]
        D = Buf.junk(pl, n * vl) if alias == "none" else bufs[idx[0 if alias == "first" else -1]]
        if c.lf == F252:
            cols = [M252.ints(d) for d in distinct]
            mult = [idx.count(j) for j in range(len(cols))]
            want = M252.words([sum(m * col[i] for m, col in zip(mult, cols)) % P252 for i in range(n)])
        else:
            want = cref.sum_columns([distinct[j] for j in idx], vl)
        arr = (ctypes.c_void_p * ncols)(*[bufs[j].ptr for j in idx])
        assert L.ms_sum_columns(h, c.lf, n, arr, ncols, D.ptr) == MS_OK
        same(D.read(), want, "sum_columns")
        for bf, d in zip(bufs, distinct):
            if bf is not D:
                same(bf.read(), d, "a column of the sum")
    else:
        raise ValueError(c.entry)


@pytest.mark.parametrize("kind,case", SWEEP)
def test_sweep(kind, case):
    run_case(backends.planner(kind), case, 1000 + CASES.index(case) * 7)


# 1, 2, 127 and 128 columns, each at a ragged length (both backends) and at a long one (device), into another buffer, cols[0] and cols[last]
SUM_COUNTS = [Case("sum", None, f, f, n, None, None, (ncols, ("none", "first", "last")[(i + j) % 3]), n > 257, ("emu", "hip") if n == 257 else ("hip",))
              for f in (FP, FQ3, F252) for j, n in enumerate((257, lengths_of("sum", None, f, f)[1][2])) for i, ncols in enumerate((1, 2, 127, 128))]


@pytest.mark.parametrize("kind,case", [pytest.param(kind, c, id=kind + "-" + case_id(c), marks=[pytest.mark.gpu] if kind == "hip" else [])
                                       for c in SUM_COUNTS for kind in c.kinds])
def test_sum_column_counts(kind, case):
    run_case(backends.planner(kind), case, 9000 + SUM_COUNTS.index(case) * 5)


# ------------------------------------------------------------------------------------------------------------------
# coverage, shown: the table of kernel templates, and the profiler's labels
# ------------------------------------------------------------------------------------------------------------------
LONG1, LONG3, LONG4 = CAP + (1 << 18) + 13, (1 << 19) + 77, (1 << 19) + 77
# template (as template_of names it) -> (entry, op, lhs field, rhs field, a length past the cap, a length with n % 256 != 0).
# Built by hand from the dispatch branches of ms_stage.cpp; a new branch there needs a row here.  k_binary<Fq3T,Fq3T,0> is instantiated but
# never launched (Fq3 + Fq3 takes the component-wise route).  The per-element inverses k_unary<*,1> are only launched below 4096 elements.
TEMPLATES = {
    "k_binary<FpT,FpT,0> over 3n words (Fq3 + Fq3)": ("binary", ADD, FQ3, FQ3, LONG3, 257),
    "k_binary<Fp252T,Fp252T,0>": ("binary", ADD, F252, F252, LONG1, 257),
    "k_binary<Fp252T,Fp252T,1>": ("binary", MUL, F252, F252, LONG1, 257),
    "k_binary<FpT,FpT,0>": ("binary", ADD, FP, FP, LONG1, 257),
    "k_binary<FpT,FpT,1>": ("binary", MUL, FP, FP, LONG1, 257),
    "k_binary<Fq3T,Fq3T,1>": ("binary", MUL, FQ3, FQ3, LONG1, 257),
    "k_binary<Fq3T,FpT,0>": ("binary", ADD, FQ3, FP, LONG1, 257),
    "k_binary<Fq3T,FpT,1>": ("binary", MUL, FQ3, FP, LONG1, 257),
    "k_binary_const<FpT,FpT,1> over 3n words (Fq3 * Fp const)": ("const", MUL, FQ3, FP, LONG3, 257),
    "k_binary_const<Fp252T,Fp252T,0>": ("const", ADD, F252, F252, LONG1, 257),
    "k_binary_const<Fp252T,Fp252T,1>": ("const", MUL, F252, F252, LONG1, 257),
    "k_binary_const<FpT,FpT,0>": ("const", ADD, FP, FP, LONG1, 257),
    "k_binary_const<FpT,FpT,1>": ("const", MUL, FP, FP, LONG1, 257),
    "k_binary_const<Fq3T,Fq3T,0>": ("const", ADD, FQ3, FQ3, LONG1, 257),
    "k_binary_const<Fq3T,Fq3T,1>": ("const", MUL, FQ3, FQ3, LONG1, 257),
    "k_binary_const<Fq3T,FpT,0>": ("const", ADD, FQ3, FP, LONG1, 257),
    "k_mul_pow<Fp252T,Fp252T>": ("mul_pow", None, F252, F252, LONG1, 257),
    "k_mul_pow<FpT,FpT>": ("mul_pow", None, FP, FP, LONG1, 257),
    "k_mul_pow<Fq3T,Fq3T>": ("mul_pow", None, FQ3, FQ3, LONG1, 257),
    "k_mul_pow<Fq3T,FpT>": ("mul_pow", None, FQ3, FP, LONG1, 257),
    "k_batch_inverse<FpT,16>": ("unary", INV, FP, FP, LONG1, 4097),
    "k_batch_inverse<Fq3T,8>": ("unary", INV, FQ3, FQ3, LONG1, 4097),
    "k_batch_inverse<Fp252T,8>": ("unary", INV, F252, F252, LONG1, 4097),
    "k_unary<Fp252T,0>": ("unary", NEG, F252, F252, LONG1, 257),
    "k_unary<Fp252T,1>": ("unary", INV, F252, F252, None, 4095),
    "k_unary<Fp252T,2>": ("unary", EXP, F252, F252, LONG1, 257),
    "k_unary<FpT,0>": ("unary", NEG, FP, FP, LONG1, 257),
    "k_unary<FpT,1>": ("unary", INV, FP, FP, None, 4095),
    "k_unary<FpT,2>": ("unary", EXP, FP, FP, LONG1, 257),
    "k_unary<FpT,0> over 3n words (-Fq3)": ("unary", NEG, FQ3, FQ3, LONG3, 257),
    "k_unary<Fq3T,1>": ("unary", INV, FQ3, FQ3, None, 4095),
    "k_unary<Fq3T,2>": ("unary", EXP, FQ3, FQ3, LONG1, 257),
    "k_convert_fp_fq3": ("convert", None, FQ3, FP, LONG1, 257),
    "hipMemcpyAsync copy route (fp)": ("convert", None, FP, FP, LONG1, 257),
    "hipMemcpyAsync copy route (fq3)": ("convert", None, FQ3, FQ3, LONG1, 257),
    "hipMemcpyAsync copy route (f252)": ("convert", None, F252, F252, LONG1, 257),
    "k_fill V=1": ("fill", None, FP, FP, LONG1, 257),
    "k_fill V=3": ("fill", None, FQ3, FQ3, LONG3, 257),
    "k_fill V=4": ("fill", None, F252, F252, LONG4, 257),
    "k_sum_columns V=1": ("sum", None, FP, FP, LONG1, 257),
    "k_sum_columns V=3": ("sum", None, FQ3, FQ3, LONG3, 257),
    "k_sum_columns252": ("sum", None, F252, F252, LONG1, 257),
}


def test_every_template_has_a_long_and_a_ragged_case():
    by_template = collections.defaultdict(list)
    for c in CASES:
        by_template[template_of(c.entry, c.op, c.lf, c.rf, c.n)].append(c)
    assert set(by_template) == set(TEMPLATES)
    for name, (entry, op, lf, rf, long_n, ragged_n) in TEMPLATES.items():
        mine = [c for c in by_template[name] if (c.entry, c.op, c.lf, c.rf) == (entry, op, lf, rf)]
        assert mine == by_template[name], name
        w = launch_words(entry, op, lf, rf)
        if long_n is None:
            assert entry == "unary" and op == INV and max(c.n for c in mine) == 4095, name     # the dispatch sends 4096 and more to k_batch_inverse
        else:
            assert long_n * w > CAP and any(c.n == long_n and "hip" in c.kinds for c in mine), name
        assert ragged_n % 256 != 0 and any(c.n == ragged_n and c.kinds == ("emu", "hip") for c in mine), name
    # every small length and every tile edge runs on both backends for every form; every long length runs on the device
    for entry, op, lf, rf in _forms():
        short, longs = lengths_of(entry, op, lf, rf)
        mine = [c for c in CASES if (c.entry, c.op, c.lf, c.rf) == (entry, op, lf, rf)]
        assert [c.n for c in mine if c.kinds == ("emu", "hip") and not c.long] == short
        assert [c.n for c in mine if c.long] == longs and all("hip" in c.kinds for c in mine)
        if entry in ("binary", "mul_pow"):
            assert {shifts_of(c.n).index(c.shift) for c in mine} == set(range(13))
        if mine[0].e is not None:
            assert {c.e for c in mine} == set(EXPONENTS)
            assert {c.e for c in mine if c.n < (1 << 13)} == set(EXPONENTS)
        if entry == "sum":
            assert {c.extra[0] for c in mine} == {1, 2, 127, 128} and {c.extra[1] for c in mine} == {"none", "first", "last"}
            assert any(c.long and c.extra[0] >= 127 for c in mine) and any(c.n % 256 and c.extra[0] >= 127 for c in mine)


STAGE_LABELS = {"stage_add", "stage_mul", "stage_add_const", "stage_mul_const", "stage_mul_pow", "stage_neg", "stage_inverse", "stage_exp",
                "stage_convert", "stage_fill", "sum_columns"}
KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("kind", KINDS)
def test_profiler_sees_every_stage_label(kind):
    """the sweep's own cases at n = 257 and 4097, one per form, under pl.profile(True): every ProfScope label of ms_stage.cpp's stages shows up"""
    pl = backends.planner(kind)
    pl.profile(True)
    try:
        for i, c in enumerate(CASES):
            if c.n in (257, 4097):
                run_case(pl, c, 5000 + i)
        seen = set(pl.profile_read())
    finally:
        pl.profile(False)
    assert STAGE_LABELS <= seen, STAGE_LABELS - seen


# ------------------------------------------------------------------------------------------------------------------
# the Goldilocks reference itself, against big integers
# ------------------------------------------------------------------------------------------------------------------
def _elems(words, v):
    xs = [PF.GL.from_mont(int(w)) for w in words]
    return xs if v == 1 else [tuple(xs[i:i + 3]) for i in range(0, len(xs), 3)]


def _words(elems, v):
    flat = elems if v == 1 else [x for t in elems for x in t]
    return np.array([PF.GL.to_mont(x) for x in flat], dtype=np.uint64)


def test_cref_stage_functions_against_big_integers():
    n = 37
    G, Q = PF.GL, PF.FQ3
    for lf, rf in PAIRS[:3]:
        vl, vr = V[lf], V[rf]
        a, b = gl_values(n, vl, 1), gl_values(n, vr, 2)
        A, B = _elems(a, vl), _elems(b, vr)
        lift = (lambda y: y) if vl == vr else Q.embed
        add = G.add if vl == 1 else Q.add
        mul = G.mul if vl == 1 else Q.mul
        powr = G.pow if vr == 1 else Q.pow
        for shift in (0, 5, -3, n, LONG_MIN):
            Br = rot(B, shift)
            assert np.array_equal(cref.binary(ADD, vl, vr, a, b, shift), _words([add(x, lift(y)) for x, y in zip(A, Br)], vl))
            assert np.array_equal(cref.binary(MUL, vl, vr, a, b, shift), _words([mul(x, lift(y)) for x, y in zip(A, Br)], vl))
            for e in EXPONENTS:
                assert np.array_equal(cref.mul_pow(vl, vr, a, b, e, shift), _words([mul(x, lift(powr(y, e))) for x, y in zip(A, Br)], vl)), (lf, rf, e)
        k = gl_values(1, vr, 3)
        K = lift(_elems(k, vr)[0])
        assert np.array_equal(cref.binary_const(ADD, vl, vr, a, k), _words([add(x, K) for x in A], vl))
        assert np.array_equal(cref.binary_const(MUL, vl, vr, a, k), _words([mul(x, K) for x in A], vl))
    for f, F in ((FP, G), (FQ3, Q)):
        v = V[f]
        a = gl_values(n, v, 4)
        A = _elems(a, v)
        zero = 0 if v == 1 else (0, 0, 0)
        assert A[-1] == zero
        assert np.array_equal(cref.unary(NEG, v, a, 0), _words([F.neg(x) for x in A], v))
        assert np.array_equal(cref.unary(INV, v, a, 0), _words([zero if x == zero else F.inv(x) for x in A], v))
        for e in EXPONENTS:
            want = _words([F.pow(x, e) for x in A], v)
            assert np.array_equal(cref.unary(EXP, v, a, e), want), (f, e)
            assert np.array_equal(want[-v:], zero_power(f, e))                 # 0^0 = 1, 0^e = 0
        if v == 1:
            assert int(cref.unary(EXP, 1, a, (1 << 32) - 1)[0]) == G.to_mont(pow(G.from_mont(int(a[0])), (1 << 32) - 1, P))
        cols = [gl_values(n, v, 10 + i) for i in range(5)]
        C = [_elems(c, v) for c in cols]
        tot = [x for x in C[0]]
        for col in C[1:]:
            tot = [(F.add(x, y)) for x, y in zip(tot, col)]
        assert np.array_equal(cref.sum_columns(cols, v), _words(tot, v))


def test_m252_helpers_against_canonical_arithmetic():
    # the Montgomery-word helpers against plain arithmetic on canonical integers (oracle.pyref.fields.F252)
    F = PF.F252
    xs = [0, 1, 2, P252 - 1, 12345678901234567890123456789 % P252, P252 >> 1]
    w = [F.to_mont(x) for x in xs]
    assert M252.R == F.R and M252.ints(ONE[F252])[0] == F.to_mont(1)
    for x, wx in zip(xs, w):
        assert M252.neg(wx) == F.to_mont(F.neg(x))
        assert M252.inv(wx) == (0 if x == 0 else F.to_mont(F.inv(x)))
        for y, wy in zip(xs, w):
            assert M252.add(wx, wy) == F.to_mont(F.add(x, y)) and M252.mul(wx, wy) == F.to_mont(F.mul(x, y))
        for e in EXPONENTS:
            assert M252.pow(wx, e) == F.to_mont(pow(x, e, P252))
    assert M252.ints(M252.words(w)) == w


# ------------------------------------------------------------------------------------------------------------------
# zero powers, refused field pairs, column counts, n == 0
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lf,rf", PAIRS)
def test_zero_to_the_zero_is_one(kind, lf, rf):
    pl = backends.planner(kind)
    L, h, n = pl.lib, pl.handle, 65
    vl, vr = V[lf], V[rf]
    a, z = values(lf, n, 77), np.zeros(n * vr, dtype=np.uint64)
    for e in EXPONENTS:
        A, Z, D = Buf(pl, a), Buf(pl, z), Buf.junk(pl, n * vl)
        assert L.ms_mul_pow(h, lf, rf, n, D.ptr, A.ptr, Z.ptr, e, 3) == MS_OK
        same(D.read(), a if e == 0 else np.zeros(n * vl, dtype=np.uint64), f"lhs * 0^{e}")
        if lf == rf:
            assert L.ms_unary(h, EXP, lf, n, D.ptr, Z.ptr, e) == MS_OK
            same(D.read(), np.tile(zero_power(lf, e), n), f"0^{e}")
            assert L.ms_unary(h, EXP, lf, n, Z.ptr, Z.ptr, e) == MS_OK
            same(Z.read(), np.tile(zero_power(lf, e), n), f"0^{e} in place")


@pytest.mark.parametrize("kind", KINDS)
def test_refused_field_pairs_and_column_counts(kind):
    pl = backends.planner(kind)
    L, h, n = pl.lib, pl.handle, 64
    before = np.arange(n * 4, dtype=np.uint64)
    A, B, D = Buf(pl, before), Buf(pl, before), Buf(pl, before)
    k = np.ones(4, dtype=np.uint64)
    for lf, rf in REFUSED_PAIRS:
        assert L.ms_binary(h, ADD, lf, rf, n, D.ptr, A.ptr, B.ptr, 0) == MS_ERR_UNSUPPORTED
        assert L.ms_binary_const(h, MUL, lf, rf, n, D.ptr, A.ptr, k.ctypes.data) == MS_ERR_UNSUPPORTED
        assert L.ms_mul_pow(h, lf, rf, n, D.ptr, A.ptr, B.ptr, 3, 0) == MS_ERR_UNSUPPORTED
        assert L.ms_convert(h, lf, rf, n, D.ptr, A.ptr) == MS_ERR_UNSUPPORTED
    for f in (FP, FQ3, F252):
        arr = (ctypes.c_void_p * 129)(*([A.ptr, B.ptr] * 64 + [A.ptr]))
        assert L.ms_sum_columns(h, f, n, arr, 0, D.ptr) == MS_ERR_INVALID
        assert L.ms_sum_columns(h, f, n, arr, 129, D.ptr) == MS_ERR_UNSUPPORTED
    pl.sync()
    for b in (A, B, D):
        same(b.read(), before, "a buffer of a refused call")


@pytest.mark.parametrize("kind", KINDS)
def test_zero_length_touches_nothing(kind):
    pl = backends.planner(kind)
    L, h = pl.lib, pl.handle
    before = np.arange(64, dtype=np.uint64)
    A, B, D = Buf(pl, before), Buf(pl, before), Buf(pl, before)
    k = np.ones(4, dtype=np.uint64)
    arr = (ctypes.c_void_p * 2)(A.ptr, B.ptr)
    for lf, rf in PAIRS:
        assert L.ms_binary(h, MUL, lf, rf, 0, D.ptr, A.ptr, B.ptr, 5) == MS_OK
        assert L.ms_binary(h, ADD, lf, rf, 0, D.ptr, D.ptr, D.ptr, 5) == MS_OK
        assert L.ms_binary_const(h, ADD, lf, rf, 0, D.ptr, A.ptr, k.ctypes.data) == MS_OK
        assert L.ms_mul_pow(h, lf, rf, 0, D.ptr, A.ptr, B.ptr, 3, LONG_MIN) == MS_OK
        assert L.ms_convert(h, lf, rf, 0, D.ptr, A.ptr) == MS_OK
    for f in (FP, FQ3, F252):
        for op in (NEG, INV, EXP):
            assert L.ms_unary(h, op, f, 0, D.ptr, A.ptr, 3) == MS_OK
        assert L.ms_fill(h, f, 0, D.ptr, k.ctypes.data) == MS_OK
        assert L.ms_sum_columns(h, f, 0, arr, 2, D.ptr) == MS_OK
    pl.sync()
    for b in (A, B, D):
        same(b.read(), before, "a buffer of a call with n = 0")


# ------------------------------------------------------------------------------------------------------------------
# aliasing: refused shapes are refused before anything is enqueued; allowed shapes give the oracle's words
# ------------------------------------------------------------------------------------------------------------------
N_AL = 300     # elements; the arena below holds four 252-bit columns of that length


def _arena(pl, seed=3):
    words = gl_values(4 * N_AL * 4, 1, seed)
    words[3::4] &= np.uint64((1 << 59) - 1)            # canonical as 252-bit elements too
    return Buf(pl, words), words


def _refused_shapes():
    """(name, call(L, h, base) -> rc): pointers are byte offsets into one arena; col(k) is the k-th of four disjoint columns of N_AL 32-byte elements."""
    n = N_AL
    col = lambda k: k * n * 32
    k = np.ones(4, dtype=np.uint64)
    out = []
    for name, fn in (("ms_binary", lambda L, h, lf, rf, d, l, r, sh: L.ms_binary(h, MUL, lf, rf, n, d, l, r, sh)),
                     ("ms_mul_pow", lambda L, h, lf, rf, d, l, r, sh: L.ms_mul_pow(h, lf, rf, n, d, l, r, 3, sh))):
        def add(what, lf, rf, d, l, r, sh, fn=fn, name=name):
            out.append((f"{name}: {what}", lambda L, h, b: fn(L, h, lf, rf, b + d, b + l, b + r, sh)))
        add("dst = lhs + 8 bytes", FP, FP, col(0) + 8, col(0), col(1), 0)
        add("dst = lhs - one element, Fq3", FQ3, FQ3, col(0), col(0) + 24, col(1), 0)
        add("dst = lhs + one element, Fp252", F252, F252, col(0) + 32, col(0), col(1), 0)
        add("dst ends inside lhs", FP, FP, col(0), col(0) + 8 * (n - 1), col(1), 0)
        add("dst == lhs == rhs, shift 1", FP, FP, col(0), col(0), col(0), 1)
        add("dst == rhs, shift 1", FP, FP, col(0), col(1), col(0), 1)
        add("dst == lhs == rhs, shift n + 1", FQ3, FQ3, col(0), col(0), col(0), n + 1)
        add("dst == rhs, shift -1, Fp252", F252, F252, col(0), col(1), col(0), -1)
        add("dst == rhs, shift LONG_MIN", FP, FP, col(0), col(1), col(0), LONG_MIN)      # LONG_MIN mod 300 = 292
        add("Fq3 dst at the address of an Fp rhs, shift 0", FQ3, FP, col(0), col(1), col(0), 0)
        add("Fq3 dst == lhs at the address of an Fp rhs", FQ3, FP, col(0), col(0), col(0), 0)
        add("dst = rhs + 8 bytes, shift 0", FP, FP, col(0) + 8, col(1), col(0), 0)
        add("Fp rhs inside an Fq3 dst, shift 0", FQ3, FP, col(0), col(1), col(0) + 16 * n, 0)
    for op in (ADD, MUL):
        for lf, rf, off in ((FP, FP, 8), (FQ3, FP, -24), (F252, F252, 32), (FQ3, FQ3, 24 * (n - 1))):
            out.append((f"ms_binary_const op {op}: dst = lhs {off:+d} bytes, fields {lf},{rf}",
                        lambda L, h, b, op=op, lf=lf, rf=rf, off=off: L.ms_binary_const(h, op, lf, rf, n, b + col(1) + off, b + col(1), k.ctypes.data)))
    for op in (NEG, INV, EXP):
        for f, off in ((FP, 8), (FQ3, -24), (F252, 32), (FP, 8 * (n - 1))):
            out.append((f"ms_unary op {op}: dst = src {off:+d} bytes, field {f}",
                        lambda L, h, b, op=op, f=f, off=off: L.ms_unary(h, op, f, n, b + col(1) + off, b + col(1), 3)))
    for f, off in ((FP, 8), (FQ3, -24), (F252, 32), (FP, -8 * (n - 1))):
        out.append((f"ms_convert: equal fields {f}, dst = src {off:+d} bytes",
                    lambda L, h, b, f=f, off=off: L.ms_convert(h, f, f, n, b + col(1) + off, b + col(1))))
    for what, d, s in (("dst == src", col(0), col(0)), ("src inside dst", col(0), col(0) + 16 * n), ("dst starts inside src", col(0) + 8 * (n - 1), col(0)),
                       ("src starts in the last element of dst", col(0), col(0) + 24 * n - 8)):
        out.append((f"ms_convert Fp -> Fq3: {what}", lambda L, h, b, d=d, s=s: L.ms_convert(h, FQ3, FP, n, b + d, b + s)))
    for f, which, off in ((FP, 1, 8), (FQ3, 0, -24), (F252, 2, 32), (FP, 2, 8 * (n - 1))):
        def sum_call(L, h, b, f=f, which=which, off=off):
            arr = (ctypes.c_void_p * 3)(b + col(0) + 64, b + col(1) + 64, b + col(2) + 64)
            return L.ms_sum_columns(h, f, n, arr, 3, b + col(which) + 64 + off)
        out.append((f"ms_sum_columns: dst = cols[{which}] {off:+d} bytes, field {f}", sum_call))
    return out


REFUSED = _refused_shapes()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", range(len(REFUSED)), ids=[name.replace(" ", "_") for name, _ in REFUSED])
def test_overlapping_buffers_are_refused(kind, shape):
    pl = backends.planner(kind)
    arena, before = _arena(pl)
    name, call = REFUSED[shape]
    rc = call(pl.lib, pl.handle, arena.ptr)
    msg = pl.lib.ms_last_error().decode()
    assert rc == MS_ERR_INVALID, f"{name}: returned {rc}"         # the return code and stop: an accepted call's output is never looked at
    assert "overlap" in msg and name.split(":")[0].split(" ")[0] in msg, msg
    pl.sync()
    same(arena.read(), before, "the arena after a refused call")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lf,rf", PAIRS)
def test_allowed_aliasing_gives_the_oracles_words(kind, lf, rf):
    pl = backends.planner(kind)
    L, h, n = pl.lib, pl.handle, N_AL
    vl, vr = V[lf], V[rf]
    a, b = values(lf, n, 21), values(rf, n, 22)
    junk = np.full(n * vl, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    for sh in (0, 7):
        # three columns that touch: lhs | dst | rhs, each starting where the one before ends
        X = Buf(pl, np.concatenate([a, junk, b]))
        assert L.ms_binary(h, MUL, lf, rf, n, X.ptr + 8 * n * vl, X.ptr, X.ptr + 16 * n * vl, sh) == MS_OK
        same(X.read(), np.concatenate([a, ref_binary(MUL, lf, rf, a, b, sh), b]), "adjacent columns")
        X = Buf(pl, np.concatenate([a, junk, b]))
        assert L.ms_mul_pow(h, lf, rf, n, X.ptr + 8 * n * vl, X.ptr, X.ptr + 16 * n * vl, 2, sh) == MS_OK
        same(X.read(), np.concatenate([a, ref_mul_pow(lf, rf, a, b, 2, sh), b]), "adjacent columns, mul_pow")
    if lf == rf:
        for sh in (0, n, -2 * n):                                  # dst == rhs (not lhs) with a shift that normalises to 0
            A, B = Buf(pl, a), Buf(pl, b)
            assert L.ms_binary(h, ADD, lf, rf, n, B.ptr, A.ptr, B.ptr, sh) == MS_OK
            same(B.read(), ref_binary(ADD, lf, rf, a, b, 0), "dst == rhs"); same(A.read(), a, "lhs")
            S = Buf(pl, a)
            assert L.ms_mul_pow(h, lf, rf, n, S.ptr, S.ptr, S.ptr, 2, sh) == MS_OK
            same(S.read(), ref_mul_pow(lf, rf, a, a, 2, 0), "cubing in place")
        k = values(lf, 1, 23)
        X = Buf(pl, np.concatenate([a, junk]))
        assert L.ms_binary_const(h, ADD, lf, rf, n, X.ptr + 8 * n * vl, X.ptr, k.ctypes.data) == MS_OK
        assert L.ms_unary(h, NEG, lf, n, X.ptr, X.ptr + 8 * n * vl, 0) == MS_OK
        want = ref_const(ADD, lf, rf, a, k)
        same(X.read(), np.concatenate([ref_unary(NEG, lf, want, 0), want]), "adjacent columns, const then neg")
        X = Buf(pl, np.concatenate([a, junk]))
        assert L.ms_convert(h, lf, lf, n, X.ptr + 8 * n * vl, X.ptr) == MS_OK
        assert L.ms_convert(h, lf, lf, n, X.ptr, X.ptr) == MS_OK
        same(X.read(), np.concatenate([a, a]), "copy into the adjacent column")
        X = Buf(pl, np.concatenate([a, b, a]))
        arr = (ctypes.c_void_p * 4)(X.ptr, X.ptr + 8 * n * vl, X.ptr, X.ptr + 16 * n * vl)
        assert L.ms_sum_columns(h, lf, n, arr, 4, X.ptr + 8 * n * vl) == MS_OK       # dst == cols[1]; cols[0] == cols[2]
        three_a = ref_binary(ADD, lf, lf, ref_binary(ADD, lf, lf, a, a, 0), a, 0)
        same(X.read(), np.concatenate([a, ref_binary(ADD, lf, lf, three_a, b, 0), a]), "sum into one of its columns")
    if (lf, rf) == (FQ3, FP):
        X = Buf(pl, np.concatenate([b, junk]))
        assert L.ms_convert(h, FQ3, FP, n, X.ptr + 8 * n, X.ptr) == MS_OK
        emb = np.zeros((n, 3), dtype=np.uint64); emb[:, 0] = b
        same(X.read(), np.concatenate([b, emb.reshape(-1)]), "embedding into the adjacent column")
