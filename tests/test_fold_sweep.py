"""Sweep of the FRI fold through the C ABI: ms_fri_fold, ms_fri_fold_rows and ms_fri_fold_dev over Fp, Fq3 and Fp252, folding factors 2, 4,
8 and 16, on the simulator and on the device, every output word compared bit for bit.

The reference is tests/fold_ref.py: the fold of one chunk by Lagrange interpolation on Python integers, which needs the chunk and its position
only -- so a shard of a layer far too large to hold has a reference too.  test_reference_equals_the_whole_layer_references pins it to the two
whole-layer restatements of apply_drp (oracle.pyref.fri.apply_drp and the C oracle's fri_fold).

What the kernels decide by position (csrc/fri_kernels.h, csrc/fp252_kernels.h, fri_fold_impl in csrc/ms_stage.cpp):
  * lane c of a shard folds chunk c0 + c of the layer: x_i^-1 is looked up at i = bitrev(c0 + c), lanes at and past `count` return;
  * Goldilocks: the table of powers of w^-1 is two-level, split at 2^12: layers below 2^12 evaluations borrow the table of the 2^12 plan
    (index shifted left by tshift = 12 - log_n), larger ones multiply by tw_hi[e >> 12] whenever e >> 12 is not zero;
  * Fp252: the table is split at 2^21, so its far half is read from log2(n / ff) >= 22 on only;
  * a layer of one chunk (log_m == 0) takes i = 0 without a bit reversal.
Every call here writes into a buffer of nchunks + 256 elements filled with a sentinel: the 256 elements behind the output must still hold it
afterwards, and the input must come back unchanged."""
import ctypes

import numpy as np
import pytest

from oracle import cref
from oracle.pyref import fri as pyfri
from oracle.pyref.fields import FQ3 as PY_FQ3
from tests import backends, fold_ref as R
from tests.fold_ref import FP, FP252, FQ3, WORDS
from ministark_amd import GpuVec
from ministark_amd.api import _offset_words

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = [pytest.param(f, id=R.NAME[f]) for f in R.FIELDS]
FACTORS = [2, 4, 8, 16]
SENTINEL = 0xA5C3_5A3C_DEAD_F01D
GUARD = 256                                              # elements behind the output that no lane may touch
SIZE_MAX = ctypes.c_size_t(-1).value
MS_ERR_INVALID, MS_ERR_UNSUPPORTED = -1, -2
BIG_OFFSET = 0x2F1E_3D4C_5B6A_7988                       # 62 bits


def generator(field):
    """the coset offset the provers use besides 1: the field's generator"""
    return 3 if field == FP252 else 7


def p_of(field):
    return R.BASE[field].p


def random_alpha(field, seed):
    return R.values(field, "random", 1, seed)


def call(pl, entry, field, log_n, ff, alpha, offset, src_ptr, out_ptr, first_chunk=0, nchunks=0):
    """one of the three entry points -> its return code; alpha: Montgomery words; offset: canonical integer.  The device alpha of "dev" lives
    until the call's work is done (the caller downloads right after)."""
    L, off = pl.lib, _offset_words(field, offset)
    alpha = np.ascontiguousarray(alpha, dtype=np.uint64)
    if entry == "rows":
        return L.ms_fri_fold_rows(pl.handle, field, log_n, ff, alpha.ctypes.data, off.ctypes.data, first_chunk, nchunks, src_ptr, out_ptr)
    if entry == "dev":
        d_alpha = GpuVec.from_numpy(pl, alpha, field)
        rc = L.ms_fri_fold_dev(pl.handle, field, log_n, ff, d_alpha.ptr, off.ctypes.data, src_ptr, out_ptr)
        pl.sync()
        return rc
    assert entry == "whole", entry
    return L.ms_fri_fold(pl.handle, field, log_n, ff, alpha.ctypes.data, off.ctypes.data, src_ptr, out_ptr)


def fold(pl, entry, field, log_n, ff, alpha, offset, src_words, first_chunk=0):
    """`src_words` (a whole layer, or for "rows" the chunks from first_chunk on) folded -> the output's words.  The guards of every call: the
    GUARD elements behind the output keep the sentinel, the input keeps its words."""
    V = WORDS[field]
    nchunks, rest = divmod(src_words.size, V * ff)
    assert rest == 0
    src = GpuVec.from_numpy(pl, src_words, field)
    out = GpuVec.from_numpy(pl, np.full((nchunks + GUARD) * V, SENTINEL, dtype=np.uint64), field)
    pl.lib.check(call(pl, entry, field, log_n, ff, alpha, offset, src.ptr, out.ptr, first_chunk, nchunks))
    got, kept = out.to_numpy(), src.to_numpy()
    src.free()
    out.free()
    assert (got[nchunks * V:] == SENTINEL).all(), f"{entry}: written behind element {nchunks} of the output (first_chunk={first_chunk})"
    assert np.array_equal(kept, src_words), f"{entry}: the input changed"
    return got[:nchunks * V]


def shard_of(layer_words, field, ff, first_chunk, nchunks):
    k = WORDS[field] * ff
    assert k * (first_chunk + nchunks) <= layer_words.size
    return layer_words[k * first_chunk:k * (first_chunk + nchunks)]


def reference(field, log_n, ff, offset, alpha):
    return R.fold(field, log_n, ff, offset % p_of(field), tuple(int(x) for x in alpha))


# ------------------------------------------------------------------------------------------------------------------
# 0. the per-chunk reference itself (no backend)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", FACTORS)
@pytest.mark.parametrize("field", FIELDS)
def test_reference_equals_the_whole_layer_references(field, ff):
    """Whole layers of 2^log_ff .. 2^(log_ff + 4) evaluations -- one chunk to sixteen -- folded chunk by chunk equal apply_drp in Python integers
    (all fields) and the C oracle (Fp, Fq3) in every word; offsets 1, the generator, p - 1 and a 62-bit value, the contents random and the edge
    patterns (0, p - 1 and 1 among them)."""
    V, p, log_ff = WORDS[field], p_of(field), ff.bit_length() - 1
    offsets = [1, generator(field), p - 1, BIG_OFFSET, 3 if field != FP252 else 7]
    for k, log_n in enumerate(range(log_ff, log_ff + 5)):
        n, offset = 1 << log_n, offsets[k]
        for pattern in ("random",) + R.PATTERNS:
            layer = R.values(field, pattern, n, seed=100 * ff + log_n)
            alpha = random_alpha(field, seed=7 * ff + log_n)
            got = reference(field, log_n, ff, offset, alpha).rows(layer)
            ext = PY_FQ3 if field == FQ3 else None
            want = pyfri.apply_drp(R.BASE[field], ext, R.elements(field, layer), offset, R.elements(field, alpha)[0], ff)
            assert np.array_equal(got, R.words(field, want)), (log_n, pattern, "apply_drp in integers")
            if field != FP252:
                assert np.array_equal(got, cref.fri_fold(layer, log_n, V, ff, alpha, offset)), (log_n, pattern, "C oracle")
            if pattern == "random":                      # and the closed form of alpha = 0, which the device tests lean on
                zero = np.zeros(V, dtype=np.uint64)
                assert np.array_equal(reference(field, log_n, ff, offset, zero).rows(layer), R.chunk_sums(field, layer, ff)), log_n


# ------------------------------------------------------------------------------------------------------------------
# a. shards at the block edges
# ------------------------------------------------------------------------------------------------------------------
def edge_shards(m):
    """(first_chunk, nchunks) around the 256-lane workgroups of a layer of m chunks.  The shard from m / 2 - 3 on is meant to be 519 chunks
    long (two workgroups and seven lanes); in the 1024 chunks of the layers here only 515 are left behind chunk 509 (two workgroups and three
    lanes), and the full 519 are one of the ranges that must be refused."""
    return [(0, 1), (0, 255), (0, 256), (0, 257), (1, 256), (255, 2), (256, 256), (m // 2 - 3, min(519, m // 2 + 3)), (m - 257, 257), (m - 1, 1)]


@pytest.mark.parametrize("ff", FACTORS)
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", KINDS)
def test_shards_at_the_block_edges(kind, field, ff):
    """A layer of 1024 chunks (2^11 .. 2^14 evaluations: for Goldilocks the borrowed table with tshift = 1 at 2^11, the layer's own from 2^12
    on; with 1024 chunks every index stays below 2^12, so tw_hi is not read here but in the 2^24 shards below) and shards that start and
    end next to a workgroup's border: one lane, 255, 256, 257, a start one past and one before a border, a shard across the middle of the
    layer, one that ends on the last chunk, the last chunk alone.  Each against the per-chunk reference and against the same chunks of
    ms_fri_fold; offsets 1 and the generator in turn."""
    pl = backends.planner(kind)
    V, log_n, m = WORDS[field], 10 + ff.bit_length() - 1, 1024
    layer = R.values(field, "random", 1 << log_n, seed=31 * ff + field)
    alpha = random_alpha(field, seed=32 * ff + field)
    offsets = (1, generator(field))
    whole = {h: fold(pl, "whole", field, log_n, ff, alpha, h, layer) for h in offsets}
    for k, (first, cnt) in enumerate(edge_shards(m)):
        h = offsets[k % 2]
        got = fold(pl, "rows", field, log_n, ff, alpha, h, shard_of(layer, field, ff, first, cnt), first)
        want = reference(field, log_n, ff, h, alpha).rows(shard_of(layer, field, ff, first, cnt), first)
        assert np.array_equal(got, want), f"chunks [{first}, {first + cnt}) offset {h}: not the reference's words"
        assert np.array_equal(got, whole[h][V * first:V * (first + cnt)]), f"chunks [{first}, {first + cnt}) offset {h}: not ms_fri_fold's words"
    for j, h in enumerate(offsets):                      # the whole-layer call over every chunk a shard above covered with this offset
        ref = reference(field, log_n, ff, h, alpha)
        have = sorted({c for k, (first, cnt) in enumerate(edge_shards(m)) if k % 2 == j for c in range(first, first + cnt)})
        assert np.array_equal(whole[h].reshape(m, V)[have].ravel(), ref.at(layer, have)), f"ms_fri_fold, offset {h}"
    # 519 chunks from m / 2 - 3 on would end four chunks behind the layer: refused, nothing written
    src = GpuVec.from_numpy(pl, shard_of(layer, field, ff, m // 2 - 3, m // 2 + 3), field)
    blank = np.full(519 * V, SENTINEL, dtype=np.uint64)
    out = GpuVec.from_numpy(pl, blank, field)
    assert call(pl, "rows", field, log_n, ff, alpha, 1, src.ptr, out.ptr, m // 2 - 3, 519) == MS_ERR_INVALID
    assert "outside the layer" in pl.lib.ms_last_error().decode() and np.array_equal(out.to_numpy(), blank)
    src.free()
    out.free()


# ------------------------------------------------------------------------------------------------------------------
# b. the smallest layers
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", FACTORS)
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_smallest_layers(kind, field, ff):
    """1, 2 and 4 chunks (the first: log_m == 0, no bit reversal to take): the whole layer through all three entry points and every split
    into shards of one chunk, against the reference"""
    pl = backends.planner(kind)
    V, log_ff = WORDS[field], ff.bit_length() - 1
    for k, log_n in enumerate((log_ff, log_ff + 1, log_ff + 2)):
        m = 1 << k
        offset = (generator(field), 1, BIG_OFFSET)[k]
        layer = R.values(field, "random", 1 << log_n, seed=51 * ff + log_n)
        alpha = random_alpha(field, seed=52 * ff + log_n)
        want = reference(field, log_n, ff, offset, alpha).rows(layer)
        assert want.size == m * V
        for entry in ("whole", "dev", "rows"):
            assert np.array_equal(fold(pl, entry, field, log_n, ff, alpha, offset, layer), want), (entry, log_n)
        for c in range(m):
            got = fold(pl, "rows", field, log_n, ff, alpha, offset, shard_of(layer, field, ff, c, 1), c)
            assert np.array_equal(got, want[V * c:V * (c + 1)]), (log_n, c)


# ------------------------------------------------------------------------------------------------------------------
# c. edge values
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", FACTORS)
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", KINDS)
def test_edge_values_against_the_reference(kind, field, ff):
    """64 chunks of p - 1 everywhere, of p - 1 and 0 in turn and of the boundary words; alpha = 0, 1, p - 1, a random element and one of the
    layer's own points (alpha / x_i == 1 in that chunk; Fq3: embedded); offsets 1, the generator, p - 1 and a 62-bit value.  ms_fri_fold and
    ms_fri_fold_dev against the reference in every word, and at alpha = 0 against the plain sums of the chunks."""
    pl = backends.planner(kind)
    V, p, log_n = WORDS[field], p_of(field), ff.bit_length() - 1 + 6
    k = 3 if field == FQ3 else 1                         # base-field components of an element
    layers = {pattern: R.values(field, pattern, 1 << log_n, seed=61) for pattern in R.PATTERNS}
    sums = {pattern: R.chunk_sums(field, layers[pattern], ff) for pattern in R.PATTERNS}
    for offset in (1, generator(field), p - 1, BIG_OFFSET):
        own_point = R.chunk_points(field, log_n, ff, offset, 37)[ff - 1]
        alphas = {"0": R.words(field, [R.embed(field, 0)]), "1": R.words(field, [R.embed(field, 1)]),
                  "p-1": R.words(field, [(p - 1,) * k if k == 3 else p - 1]), "random": random_alpha(field, seed=62 + ff),
                  "x_i": R.words(field, [R.embed(field, own_point)])}
        for name, alpha in alphas.items():
            ref = reference(field, log_n, ff, offset, alpha)
            for pattern in R.PATTERNS:
                want = ref.rows(layers[pattern])
                if name == "0":
                    assert np.array_equal(want, sums[pattern]), (pattern, offset)
                for entry in ("whole", "dev"):
                    got = fold(pl, entry, field, log_n, ff, alpha, offset, layers[pattern])
                    assert np.array_equal(got, want), f"{entry}: {pattern}, alpha = {name}, offset = {offset:#x}"


# ------------------------------------------------------------------------------------------------------------------
# d. shards of layers too large to hold
# ------------------------------------------------------------------------------------------------------------------
FAR_CHUNKS = 300                                         # two workgroups, the second one partial


@pytest.mark.parametrize("ff", FACTORS)
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", KINDS)
def test_shards_of_layers_too_large_to_hold(kind, field, ff):
    """300 chunks of a layer of 2^24 evaluations (Goldilocks: tw_hi indices up to 2^12 / ff) or 2^26 (Fp252: log2(n / ff) >= 22, so
    i = bitrev(chunk) reaches the table's far half, i >= 2^21, at every folding factor): the layer's first chunks, the 300 around its
    middle (bitrev swings between the smallest and the largest indices) and its last ones.  Consecutive chunks are bit-reversed all over the
    table, so each of the shards reads both halves.  Only the shard is uploaded; the per-chunk reference is the check."""
    pl = backends.planner(kind)
    log_n = 26 if field == FP252 else 24
    m = (1 << log_n) // ff
    alpha = random_alpha(field, seed=71 * ff + field)
    for k, first in enumerate((0, m // 2 - FAR_CHUNKS // 2, m - FAR_CHUNKS)):
        offset = (1, generator(field))[(k + ff.bit_length()) % 2]
        shard = R.values(field, "random", FAR_CHUNKS * ff, seed=72 * ff + k)
        if field == FP252:                               # the case is about the table's far half: the shard reads it, and the near half too
            idx = [R.bitrev(first + c, log_n - ff.bit_length() + 1) for c in range(FAR_CHUNKS)]
            assert max(idx) >= 1 << 21 > min(idx), (first, min(idx), max(idx))
        got = fold(pl, "rows", field, log_n, ff, alpha, offset, shard, first)
        want = reference(field, log_n, ff, offset, alpha).rows(shard, first)
        assert np.array_equal(got, want), f"chunks [{first}, {first + FAR_CHUNKS}) of 2^{log_n}, offset {offset}"


# ------------------------------------------------------------------------------------------------------------------
# e. whole layers above 2^16 on the device
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("field,log_n,ff,entry", [pytest.param(FQ3, 18, 2, "whole", id="fq3-2^18-ff2"), pytest.param(FQ3, 18, 16, "dev", id="fq3-2^18-ff16-dev"),
                                                  pytest.param(FP, 20, 4, "whole", id="fp-2^20-ff4"), pytest.param(FP, 20, 16, "whole", id="fp-2^20-ff16")])
def test_whole_layers_above_2_16_hip(field, log_n, ff, entry):
    """every chunk of a layer of thousands of workgroups, offsets 1 and 7, against the C oracle"""
    pl = backends.planner("hip")
    V = WORDS[field]
    layer = R.values(field, "random", 1 << log_n, seed=81 + ff)
    alpha = random_alpha(field, seed=82 + ff)
    for offset in (1, 7):
        got = fold(pl, entry, field, log_n, ff, alpha, offset, layer)
        assert np.array_equal(got, cref.fri_fold(layer, log_n, V, ff, alpha, offset)), offset


@pytest.mark.gpu
def test_whole_fp252_layer_2_18_hip():
    """2^16 chunks folded by 4 on the coset of 3: the whole layer equals its own shards put together (ragged ones, none a multiple of a
    workgroup) and the per-chunk reference at 64 positions, the first and the last chunk among them"""
    pl = backends.planner("hip")
    field, log_n, ff, offset = FP252, 18, 4, 3
    m = (1 << log_n) // ff
    layer = R.values(field, "random", 1 << log_n, seed=91)
    alpha = random_alpha(field, seed=92)
    whole = fold(pl, "whole", field, log_n, ff, alpha, offset, layer)
    cuts = [0, 300, m // 4 + 1, m // 2 - 129, m - 257, m]
    parts = [fold(pl, "rows", field, log_n, ff, alpha, offset, shard_of(layer, field, ff, a, b - a), a) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate(parts), whole)
    at = sorted({0, m - 1} | {int(c) for c in np.random.default_rng(93).integers(0, m, size=62)})
    assert np.array_equal(whole.reshape(m, 4)[at].ravel(), reference(field, log_n, ff, offset, alpha).at(layer, at))


# ------------------------------------------------------------------------------------------------------------------
# f. what ms_fri_fold_rows refuses
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", KINDS)
def test_rows_refusals_write_nothing(kind, field):
    """Chunk ranges outside the layer (the bound in its subtraction form: first_chunk + nchunks may wrap), layer sizes below the folding factor
    and above 2^32, folding factors the reference does not have, an output inside the input; and the two empty ranges that are no error.
    The output holds the sentinel after each."""
    pl, L = backends.planner(kind), backends.planner(kind).lib
    V, ff, log_ff, log_n = WORDS[field], 4, 2, 8
    m = (1 << log_n) // ff
    layer = R.values(field, "random", 1 << log_n, seed=5)
    alpha = random_alpha(field, seed=6)
    src = GpuVec.from_numpy(pl, layer, field)
    blank = np.full((m + GUARD) * V, SENTINEL, dtype=np.uint64)
    out = GpuVec.from_numpy(pl, blank, field)

    def rows(first, cnt, log_n=log_n, ff=ff):
        rc = call(pl, "rows", field, log_n, ff, alpha, 1, src.ptr, out.ptr, first, cnt)
        msg = L.ms_last_error().decode() if rc else ""
        assert np.array_equal(out.to_numpy(), blank), (first, cnt, log_n, ff, "the output was written")
        assert np.array_equal(src.to_numpy(), layer)
        return rc, msg

    for first, cnt in ((m + 1, 0), (m, 1), (1, SIZE_MAX), (1, m), (0, m + 1), (SIZE_MAX, 2)):
        rc, msg = rows(first, cnt)
        assert rc == MS_ERR_INVALID and "outside the layer" in msg, (first, cnt, rc, msg)
    for bad_log_n in (log_ff - 1, 33):
        rc, msg = rows(0, 1, log_n=bad_log_n)
        assert rc == MS_ERR_INVALID and "bad layer size" in msg, (bad_log_n, rc, msg)
    for bad_ff in (3, 32):
        rc, msg = rows(0, 1, ff=bad_ff)
        assert rc == MS_ERR_UNSUPPORTED, (bad_ff, rc, msg)
    for first in (m, 0):                                 # nothing to fold: no error, nothing written
        assert rows(first, 0) == (0, "")
    # an output that overlaps the shard it folds: refused by both entry points alike, the buffer keeps its words
    for entry, first, cnt in (("rows", 5, m // 2), ("whole", 0, m)):
        for out_ptr in (src.ptr, src.ptr + (cnt * ff - 1) * V * 8, src.ptr - (cnt - 1) * V * 8):
            rc = call(pl, entry, field, log_n, ff, alpha, 1, src.ptr, out_ptr, first, cnt)
            assert rc == MS_ERR_INVALID and "d_out overlaps d_evals" in L.ms_last_error().decode(), (entry, rc)
            assert np.array_equal(src.to_numpy(), layer)
    # ... and the same shard next to its input is folded
    got = fold(pl, "rows", field, log_n, ff, alpha, 1, shard_of(layer, field, ff, 5, m // 2), 5)
    assert np.array_equal(got, reference(field, log_n, ff, 1, alpha).rows(shard_of(layer, field, ff, 5, m // 2), 5))
    src.free()
    out.free()
