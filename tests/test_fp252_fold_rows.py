"""ms_fri_fold_rows over the 252-bit field: a layer held by rows folds shard by shard into the words ms_fri_fold gives for the whole
layer (folding factors 2, 4, 8, 16; equal and ragged splits), and the whole-layer fold equals apply_drp in Python integers."""
import numpy as np
import pytest

from oracle.pyref.fields import F252
from tests import backends
from ministark_amd import STARK252_FP, f252_from_mont_limbs, f252_to_mont_limbs
from ministark_amd.api import GpuVec, apply_drp, _offset_words

P = F252.p


def _rand_words(rng, n):
    # any four words below p are the Montgomery form of some element: top limb below 2^59 keeps the value under 2^251 < p
    w = rng.integers(0, 2 ** 64, size=(n, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64(2 ** 59 - 1)
    return w.ravel()


def _fold_rows(pl, words, log_n, ff, alpha, offset, first_chunk, nchunks):
    """chunks [first_chunk, first_chunk + nchunks) of the layer `words`, uploaded as a shard of their own"""
    L = pl.lib
    src = GpuVec.from_numpy(pl, words[4 * ff * first_chunk:4 * ff * (first_chunk + nchunks)], STARK252_FP)
    out = GpuVec(pl, nchunks, STARK252_FP)
    off = _offset_words(STARK252_FP, offset)
    L.check(L.ms_fri_fold_rows(pl.handle, STARK252_FP, log_n, ff, alpha.ctypes.data, off.ctypes.data, first_chunk, nchunks, src.ptr, out.ptr))
    return out.to_numpy()


def _cases():
    out = []
    for kind, top in (("emu", 10), ("hip", 16)):
        for ff, log_ff in ((2, 1), (4, 2), (8, 3), (16, 4)):
            for log_n in range(log_ff, top + 1):
                out.append(pytest.param(kind, ff, log_n, id=f"{kind}-ff{ff}-2^{log_n}", marks=[pytest.mark.gpu] if kind == "hip" else []))
    return out


@pytest.mark.parametrize("kind,ff,log_n", _cases())
def test_shards_concatenate_to_the_whole_fold(kind, ff, log_n):
    pl = backends.planner(kind)
    rng = np.random.default_rng(1000 * ff + log_n)
    n = 1 << log_n
    m = n // ff
    words = _rand_words(rng, n)
    alpha = np.ascontiguousarray(f252_to_mont_limbs(int.from_bytes(rng.bytes(32), "little") % P), dtype=np.uint64)
    offset = 3 if log_n % 2 else 1
    want = apply_drp(GpuVec.from_numpy(pl, words, STARK252_FP), alpha, ff, offset).to_numpy()          # ms_fri_fold
    assert want.size == 4 * m
    splits = [[m]] + [[m // s] * s for s in (2, 8) if m >= s]
    if m >= 3:
        a = m // 3
        splits.append([a, 1, m - a - 1])                      # ragged
    for parts in splits:
        got, at = [], 0
        for cnt in parts:
            got.append(_fold_rows(pl, words, log_n, ff, alpha, offset, at, cnt))
            at += cnt
        assert at == m
        assert np.array_equal(np.concatenate(got), want), parts


def _bitrev_list(v):
    bits = (len(v) - 1).bit_length()
    return [v[int(format(i, "0%db" % bits)[::-1], 2) if bits else 0] for i in range(len(v))]


def _drp_integers(evals, offset, alpha, ff):
    """apply_drp (src/fri.rs:526-567) on canonical integers: bit-reverse, inverse transform on the coset, x folding factor, chunks of
    folding_factor coefficients weighted with powers of alpha, forward transform on the folded coset, bit-reverse"""
    n = len(evals)
    nat = _bitrev_list(evals)
    w, hinv, ninv = F252.root_of_unity(n), pow(offset, -1, P), pow(n, -1, P)
    coeffs = [sum(nat[j] * pow(w, -i * j % n, P) for j in range(n)) * ninv * pow(hinv, i, P) * ff % P for i in range(n)]
    drp = [sum(coeffs[c * ff + k] * pow(alpha, k, P) for k in range(ff)) % P for c in range(n // ff)]
    m = n // ff
    wm, hm = F252.root_of_unity(m), pow(offset, ff, P)
    out = [sum(drp[i] * pow(hm * pow(wm, j, P) % P, i, P) for i in range(m)) % P for j in range(m)]
    return _bitrev_list(out)


@pytest.mark.parametrize("kind", [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("ff", [2, 4, 8, 16])
def test_rows_equal_apply_drp_in_integers(kind, ff):
    pl = backends.planner(kind)
    rng = np.random.default_rng(ff)
    log_n, offset = 6, 3
    n = 1 << log_n
    m = n // ff
    words = _rand_words(rng, n)
    a = int.from_bytes(rng.bytes(32), "little") % P
    alpha = np.ascontiguousarray(f252_to_mont_limbs(a), dtype=np.uint64)
    want = _drp_integers([f252_from_mont_limbs(r) for r in words.reshape(n, 4)], offset, a, ff)
    halves = [_fold_rows(pl, words, log_n, ff, alpha, offset, f, m // 2) for f in (0, m // 2)]
    got = [f252_from_mont_limbs(r) for r in np.concatenate(halves).reshape(m, 4)]
    assert got == want
