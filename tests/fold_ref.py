"""TEST INFRASTRUCTURE -- the FRI fold of ONE chunk, on Python integers.

`apply_drp` (src/fri.rs:526-567) folds a bit-reversed layer of n = 2^log_n evaluations on the coset h <w> by the factor ff into n / ff values.
Chunk c of the layer -- the ff consecutive elements c ff .. c ff + ff - 1 -- holds the evaluations at the ff points

    x_q = h w^(i + bitrev_{log2 ff}(q) m),    i = bitrev_{log2 m}(c),    m = n / ff,    w = root_of_unity(n),

and element c of the next layer is   ff * P_c(alpha),   P_c the polynomial of degree < ff through the ff points (x_q, value_q).  The factor ff is
the reference's `coeffs *= folding_factor`, which nothing cancels: its layers are ff times the textbook fold.

P_c(alpha) is taken here by plain Lagrange interpolation over the base field: sum_q value_q L_q(alpha) with
L_q(alpha) = prod_{r != q} (alpha - x_r) / (x_q - x_r).  An Fq3 value is three base-field values at the same point, so its three component
polynomials share the weights L_q(alpha) -- computed once per chunk -- and P_c(alpha) = sum_q L_q(alpha) * value_q in Fq3.  Nothing of this is
shared with the kernels (an inverse butterfly network and a Horner rule in alpha / x_i) or with the whole-layer references (oracle.cref.fri_fold,
oracle.pyref.fri.apply_drp: two transforms of the whole layer), which cannot fold a shard of a layer too large to hold.  The reference of a chunk
needs the chunk and its position only.

Elements cross the C ABI as Montgomery words (one per Goldilocks value, three per Fq3 element, four little-endian limbs per Fp252 element);
`elements` / `words` convert between those and canonical integers (Fq3: 3-tuples)."""
import functools

import numpy as np

from oracle.pyref.fields import F252, FQ3 as PY_FQ3, GL
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as FP252

FIELDS = (FP, FQ3, FP252)
NAME = {FP: "fp", FQ3: "fq3", FP252: "fp252"}
WORDS = {FP: 1, FQ3: 3, FP252: 4}                        # 64-bit words per element
BASE = {FP: GL, FQ3: GL, FP252: F252}                    # the field of the evaluation points, the offset and the weights' denominators
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------------------
# Montgomery words <-> canonical integers
# ------------------------------------------------------------------------------------------------------------------
def elements(field, w):
    """numpy u64 Montgomery words -> list of canonical elements: ints, or 3-tuples for Fq3"""
    w = [int(x) for x in np.asarray(w, dtype=np.uint64).ravel()]
    assert len(w) % WORDS[field] == 0
    if field == FP:
        return [GL.from_mont(x) for x in w]
    if field == FQ3:
        return [tuple(GL.from_mont(x) for x in w[k:k + 3]) for k in range(0, len(w), 3)]
    return [F252.from_mont(w[k] | w[k + 1] << 64 | w[k + 2] << 128 | w[k + 3] << 192) for k in range(0, len(w), 4)]


def words(field, elems):
    """list of canonical elements -> numpy u64 Montgomery words"""
    out = []
    for e in elems:
        if field == FP:
            out.append(GL.to_mont(e % GL.p))
        elif field == FQ3:
            out.extend(GL.to_mont(c % GL.p) for c in e)
        else:
            m = F252.to_mont(e % F252.p)
            out.extend((m >> (64 * k)) & _M64 for k in range(4))
    return np.array(out, dtype=np.uint64)


def embed(field, a):
    """a base-field integer as an element of `field`"""
    return PY_FQ3.embed(a) if field == FQ3 else a % BASE[field].p


# ------------------------------------------------------------------------------------------------------------------
# the fold of a chunk
# ------------------------------------------------------------------------------------------------------------------
def bitrev(v, bits):
    return int(format(v, "0%db" % bits)[::-1], 2) if bits else 0


def chunk_points(field, log_n, ff, offset, c):
    """the ff points x_q at which chunk c of the bit-reversed layer holds its evaluations, in the chunk's order"""
    F = BASE[field]
    log_ff = ff.bit_length() - 1
    assert ff == 1 << log_ff and log_n >= log_ff
    m = 1 << (log_n - log_ff)
    assert 0 <= c < m
    i = bitrev(c, log_n - log_ff)
    w = F.root_of_unity(1 << log_n)
    return [offset * pow(w, i + bitrev(q, log_ff) * m, F.p) % F.p for q in range(ff)]


def chunk_weights(field, log_n, ff, offset, alpha, c):
    """ff L_q(alpha), q < ff: elements of `field` (alpha is one), so that the folded value is sum_q weight_q * value_q"""
    F = BASE[field]
    p = F.p
    xs = chunk_points(field, log_n, ff, offset, c)
    if field == FQ3:
        mul, scale = PY_FQ3.mul, PY_FQ3.mul_base
        diff = [PY_FQ3.sub(alpha, PY_FQ3.embed(x)) for x in xs]
        one = PY_FQ3.one()
    else:
        mul = scale = F.mul
        diff = [(alpha - x) % p for x in xs]
        one = 1
    # prod_{r != q} (alpha - x_r) from the products of the factors before q and after q: no division, so alpha == x_q is no special case
    before, after = [one] * ff, [one] * ff
    for q in range(1, ff):
        before[q] = mul(before[q - 1], diff[q - 1])
    for q in range(ff - 2, -1, -1):
        after[q] = mul(after[q + 1], diff[q + 1])
    out = []
    for q in range(ff):
        den = 1
        for r in range(ff):
            if r != q:
                den = den * (xs[q] - xs[r]) % p
        out.append(scale(mul(before[q], after[q]), ff * F.inv(den) % p))
    return out


def weighted_sum(field, weights, values):
    if field == FQ3:
        acc = PY_FQ3.zero()
        for w, v in zip(weights, values):
            acc = PY_FQ3.add(acc, PY_FQ3.mul(w, v))
        return acc
    return sum(w * v for w, v in zip(weights, values)) % BASE[field].p


def fold_chunk(field, log_n, ff, offset, alpha, c, values):
    """element c of the next layer from the ff canonical `values` of chunk c"""
    assert len(values) == ff
    return weighted_sum(field, chunk_weights(field, log_n, ff, offset, alpha, c), values)


class Fold:
    """The fold of one layer shape with one offset and one challenge: the weights of a chunk are computed once and serve every layer content
    folded at that position (they do not depend on the evaluations).  offset: canonical integer of the base field; alpha_words: the
    Montgomery words of the challenge, as the entry points take them."""

    def __init__(self, field, log_n, ff, offset, alpha_words):
        self.field, self.log_n, self.ff, self.offset = field, log_n, ff, offset % BASE[field].p
        self.alpha = elements(field, alpha_words)[0]
        self.nchunks = (1 << log_n) // ff
        self._weights = {}

    def weights(self, c):
        if c not in self._weights:
            self._weights[c] = chunk_weights(self.field, self.log_n, self.ff, self.offset, self.alpha, c)
        return self._weights[c]

    def rows(self, shard_words, first_chunk=0):
        """Montgomery words of chunks [first_chunk, first_chunk + k) of the layer -> the words of those k elements of the next layer"""
        ev = elements(self.field, shard_words)
        assert len(ev) % self.ff == 0
        k = len(ev) // self.ff
        assert first_chunk + k <= self.nchunks
        return words(self.field, [weighted_sum(self.field, self.weights(first_chunk + j), ev[j * self.ff:(j + 1) * self.ff]) for j in range(k)])

    def at(self, layer_words, chunks):
        """the words of the next layer's elements at the positions `chunks`, from the words of a whole layer"""
        V, ff = WORDS[self.field], self.ff
        lw = np.asarray(layer_words, dtype=np.uint64)
        return words(self.field, [weighted_sum(self.field, self.weights(c), elements(self.field, lw[c * ff * V:(c + 1) * ff * V])) for c in chunks])


@functools.lru_cache(maxsize=None)
def fold(field, log_n, ff, offset, alpha_words):
    """a shared Fold (alpha_words: a tuple of ints)"""
    return Fold(field, log_n, ff, offset, np.array(alpha_words, dtype=np.uint64))


def chunk_sums(field, layer_words, ff):
    """The closed form at alpha = 0: element c of the next layer is the plain sum of the chunk's ff evaluations (ff times the constant
    coefficient of P_c).  Linear, so it holds on the Montgomery words as they are."""
    p = BASE[field].p
    if field == FP252:
        w = [int(x) for x in np.asarray(layer_words, dtype=np.uint64)]
        vals = [w[k] | w[k + 1] << 64 | w[k + 2] << 128 | w[k + 3] << 192 for k in range(0, len(w), 4)]
        out = []
        for c in range(len(vals) // ff):
            s = sum(vals[c * ff:(c + 1) * ff]) % p
            out.extend((s >> (64 * k)) & _M64 for k in range(4))
        return np.array(out, dtype=np.uint64)
    V = WORDS[field]
    a = np.asarray(layer_words, dtype=np.uint64).reshape(-1, ff, V)
    return np.array([[sum(int(x) for x in a[c, :, v]) % p for v in range(V)] for c in range(a.shape[0])], dtype=np.uint64).ravel()


# ------------------------------------------------------------------------------------------------------------------
# layer contents: the Montgomery words a kernel reads
# ------------------------------------------------------------------------------------------------------------------
PATTERNS = ("all_pm1", "alternating", "boundary")        # besides "random"


def _limbs(v):
    return [(v >> (64 * k)) & _M64 for k in range(4)]


def values(field, pattern, n, seed=0):
    """n elements of `field` as canonical words (every word / limb group below p):
      random       uniform Goldilocks words; Fp252: uniform limbs with the top one below 2^59 (any such value is below 2^251 < p)
      all_pm1      p - 1 in every word (Fp252: in every element)
      alternating  p - 1, 0, p - 1, 0, ... word by word (Fp252: element by element), as tests/test_ntt_parity.py::_adversarial pattern 1
      boundary     _adversarial's boundary words, first in order and then drawn from the list; Fp252: the digit-edge elements of
                   tests/test_fp252_parity.py and elements whose limbs are those boundary words"""
    from tests.test_ntt_parity import _adversarial
    V = WORDS[field]
    rng = np.random.default_rng(seed)
    if field != FP252:
        if pattern == "random":
            return rng.integers(0, GL.p, size=n * V, dtype=np.uint64)
        if pattern == "boundary":
            cyc, drawn = _adversarial(n, V, 2), _adversarial(n, V, 3)
            half = (n * V) // 2
            return np.concatenate([cyc[:half], drawn[half:]])
        return _adversarial(n, V, {"all_pm1": 0, "alternating": 1}[pattern])
    a = np.zeros((n, 4), dtype=np.uint64)
    pm1 = np.array(_limbs(F252.p - 1), dtype=np.uint64)
    if pattern == "random":
        a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 59) - 1)
    elif pattern == "all_pm1":
        a[:] = pm1
    elif pattern == "alternating":
        a[::2] = pm1
    else:
        assert pattern == "boundary", pattern
        from tests.test_fp252_parity import DIGIT_EDGES_252
        gl_edges = [int(x) for x in _adversarial(14, 1, 2)]
        edge = [v % F252.p for v in DIGIT_EDGES_252]
        for k in range(len(gl_edges)):                   # four consecutive boundary words as limbs, the top one cut to 59 bits
            edge.append(sum(gl_edges[(k + j) % len(gl_edges)] << (64 * j) for j in range(3)) | (gl_edges[(k + 3) % len(gl_edges)] & ((1 << 59) - 1)) << 192)
        table = np.array([_limbs(v) for v in edge], dtype=np.uint64)
        pick = rng.integers(0, len(edge), size=n)
        pick[:len(edge)] = np.arange(len(edge))[:n]
        a[:] = table[pick]
    return a.ravel()
