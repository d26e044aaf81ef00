"""The device-resident public coin (ms_coin_*, ministark_amd/coin.py) against tests/coin_ref.py: SHA-256 and BLAKE2s, every rule of
the word stream, the three reseeds, the field samplers with their rejection branches, the query sampler, the proof-of-work search and
the refusals.  The coin's state is read back (ms_coin_read) and compared after every step, not only what a step returns."""
import ctypes

import numpy as np
import pytest

from tests import backends, coin_ref
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as FP252, GpuVec, grind_proof_of_work
from ministark_amd._lib import CoinState
from ministark_amd.api import F252_P, FIELD_WORDS, GL_P, f252_to_mont_limbs, gl_to_mont
from ministark_amd.coin import PublicCoin

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
HASHES = ["sha256", "blake2s"]
SEED = bytes(range(32))


def pair(kind, hash, seed=SEED):
    return PublicCoin(backends.planner(kind), seed, hash), coin_ref.Coin(seed, hash)


def same_state(coin, ref):
    assert coin.state() == ref.state()


def draw_both(coin, ref, field, count):
    got = [int(v) for v in coin.draw(field, count).to_numpy()]
    assert got == ref.draw(field, count)
    same_state(coin, ref)
    return got


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_goldilocks_draws_cross_digest_boundaries(kind, hash):
    for count in (1, 4, 5, 9):                                     # a digest is 4 words: whole digests, and one word past a boundary
        coin, ref = pair(kind, hash)
        same_state(coin, ref)
        words = draw_both(coin, ref, FP, count)
        assert all(w < GL_P for w in words)
    draw_both(coin, ref, FP, 2)                                    # 9 + 2: continues inside the third digest


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_fq3_draws_take_c0_c1_c2_in_order(kind, hash):
    coin, ref = pair(kind, hash)
    for count in (1, 2, 3):                                        # words 0-2, then 3-8: the second draw straddles a digest
        assert len(draw_both(coin, ref, FQ3, count)) == 3 * count


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_fp252_draws_reject_about_half_the_samples(kind, hash):
    for seed in (SEED, bytes(31) + b"\x07"):
        coin, ref = pair(kind, hash, seed)
        limbs = draw_both(coin, ref, FP252, 8)
        assert ref.rejections >= 1 and ref.first_try >= 1         # both branches of the sampler were taken (p is about 2^251 of 2^252)
        for i in range(8):
            assert sum(v << (64 * k) for k, v in enumerate(limbs[4 * i: 4 * i + 4])) < F252_P


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_goldilocks_rejection_branch(kind, hash):
    """No seed reaches a word >= p in practice (2^-32 per word): plant it in the unread bytes."""
    le = lambda v: int(v).to_bytes(8, "little")
    for first, second, want in (((1 << 64) - 1, 12345, 12345), (GL_P, 777, 777), (GL_P - 1, 777, GL_P - 1)):
        coin, ref = pair(kind, hash)
        unread = le(second) + le(first)                            # consumed from the end: `first` comes out first
        coin.set_state(SEED, 3, unread)
        ref.seed, ref.counter, ref.unread = SEED, 3, unread
        same_state(coin, ref)
        assert draw_both(coin, ref, FP, 1) == [want]
        assert ref.rejections == (0 if want == first else 1)


def elements(field, count, rng):
    """Montgomery words of `count` elements that include 0, 1 and p - 1"""
    V, p = FIELD_WORDS[field], (F252_P if field == FP252 else GL_P)
    vals = [[0, 1, p - 1][(i + k) % 3] if i < 3 else int.from_bytes(rng.bytes(40), "little") % p for i in range(count) for k in range(1 if field == FP252 else V)]
    if field == FP252:
        return np.concatenate([f252_to_mont_limbs(v) for v in vals] or [np.empty(0, dtype=np.uint64)]).astype(np.uint64)
    return np.array([gl_to_mont(v) for v in vals], dtype=np.uint64)


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_reseeds(kind, hash):
    pl = backends.planner(kind)
    rng = np.random.default_rng(5)
    coin, ref = pair(kind, hash)
    draw_both(coin, ref, FP, 1)                                    # leave unread bytes and a counter behind: the reseeds must clear them
    digest = bytes(rng.bytes(32))
    d = GpuVec.from_numpy(pl, np.frombuffer(digest, dtype=np.uint64))
    coin.reseed_digest(d.ptr)
    ref.reseed_digest(digest)
    same_state(coin, ref)
    draw_both(coin, ref, FP, 3)
    for v in (0, 1, 0x0102030405060708, (1 << 64) - 1):
        coin.reseed_int(v)
        ref.reseed_int(v)
        same_state(coin, ref)
    for field in (FP, FQ3, FP252):
        for count in (0, 1, 2, 65):                                # 65: more than one wave's worth of lanes
            words = elements(field, count, rng)
            draw_both(coin, ref, FP, 1)
            before = coin.state()
            coin.reseed_elements(GpuVec.from_numpy(pl, words, field))
            ref.reseed_elements(field, words)
            same_state(coin, ref)
            if count == 0:
                assert coin.state() == before and before["unread"]              # not even counter or unread bytes change
            host, _ = pair(kind, hash)
            host.set_state(before["seed"], before["counter"], before["unread"])
            host.reseed_elements(words, field)                     # the host form gives the same state
            same_state(host, ref)


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_interleaved_script(kind, hash):
    pl = backends.planner(kind)
    coin, ref = pair(kind, hash, b"\xa5" * 32)
    draw_both(coin, ref, FP, 3)
    root = bytes(range(100, 132))
    coin.reseed_digest(GpuVec.from_numpy(pl, np.frombuffer(root, dtype=np.uint64)).ptr)
    ref.reseed_digest(root)
    draw_both(coin, ref, FP252, 1)
    coin.reseed_int(99)
    ref.reseed_int(99)
    draw_both(coin, ref, FP, 6)
    draw_both(coin, ref, FQ3, 1)


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_draw_queries(kind, hash):
    coin, ref = pair(kind, hash)
    for max_n, size in ((1, 2), (32, 1 << 6), (32, 1 << 20), (8, 3 << 10)):
        got, want = coin.draw_queries(max_n, size), ref.draw_queries(max_n, size)
        assert got == want and all(p < size for p in got) and got == sorted(set(got))
        same_state(coin, ref)
        if size == 1 << 6:
            assert len(want) < 32                                  # duplicates collapsed
        if size == 1 << 20:
            assert ref.rejections >= 1                             # a power-of-two range rejects about half the words
    assert coin.draw_queries(0, 16) == []
    same_state(coin, ref)


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_pow_grind_uses_the_seed_on_the_device(kind, hash):
    pl = backends.planner(kind)
    coin, ref = pair(kind, hash)
    coin.reseed_int(4)
    ref.reseed_int(4)
    for bits in (8, 12):
        nonce = coin.grind(bits)
        assert nonce == grind_proof_of_work(pl, coin.state()["seed"], bits, hash=hash)
        assert nonce == ref.grind(bits)
        same_state(coin, ref)                                      # grinding does not reseed


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_the_state_alone(kind):
    pl = backends.planner(kind)
    L, h = pl.lib, pl.handle
    coin, ref = pair(kind, "sha256")
    draw_both(coin, ref, FP, 1)
    buf = GpuVec(pl, 8, FP)
    n, out, handle = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_void_p()
    pos = (ctypes.c_uint64 * 4)()
    st = CoinState()
    ctypes.memmove(st.seed, SEED, 32)
    st.nbytes = 12
    refused = [
        L.ms_coin_create(h, 2, ctypes.create_string_buffer(SEED, 32), ctypes.byref(handle)),        # unknown hash
        L.ms_coin_create(h, 0, None, ctypes.byref(handle)),
        L.ms_coin_create(h, 0, ctypes.create_string_buffer(SEED, 32), None),
        L.ms_coin_read(h, coin.ptr, None),
        L.ms_coin_write(h, coin.ptr, None),
        L.ms_coin_write(h, coin.ptr, ctypes.byref(st)),                                              # nbytes = 12
        L.ms_coin_reseed_digest(h, coin.ptr, None),
        L.ms_coin_reseed_digest(h, None, buf.ptr),
        L.ms_coin_reseed_digest(h, buf.ptr, buf.ptr),                                                # not a coin of this context
        L.ms_coin_reseed_int(h, None, 1),
        L.ms_coin_reseed_elements(h, coin.ptr, 7, buf.ptr, 1),                                       # unknown field
        L.ms_coin_reseed_elements(h, coin.ptr, FP, None, 1),
        L.ms_coin_reseed_elements_host(h, coin.ptr, 7, buf.ptr, 1),
        L.ms_coin_reseed_elements_host(h, coin.ptr, FP, None, 1),
        L.ms_coin_draw(h, coin.ptr, 7, 1, buf.ptr),
        L.ms_coin_draw(h, coin.ptr, FP, 1, None),
        L.ms_coin_draw(h, coin.ptr, FP, 1, coin.ptr),                                                # into its own state
        L.ms_coin_draw_queries(h, coin.ptr, 4, 0, pos, ctypes.byref(n)),                             # domain_size = 0
        L.ms_coin_draw_queries(h, coin.ptr, 4, 16, None, ctypes.byref(n)),
        L.ms_coin_draw_queries(h, coin.ptr, 4, 16, pos, None),
        L.ms_coin_pow_grind(h, coin.ptr, 65, 1 << 20, ctypes.byref(out)),                            # bits > 64
        L.ms_coin_pow_grind(h, coin.ptr, 8, 1 << 20, None),
        L.ms_coin_destroy(h, buf.ptr),
    ]
    assert refused == [-1] * len(refused)                                                            # MS_ERR_INVALID
    same_state(coin, ref)


@pytest.mark.parametrize("kind", KINDS)
def test_checked_mode_scans_the_reseed_elements(kind):
    pl = backends.planner(kind)
    coin, ref = pair(kind, "sha256")
    bad = np.array([gl_to_mont(5), GL_P + 1, gl_to_mont(6)], dtype=np.uint64)
    pl.checked(True)
    try:
        for form in (lambda: coin.reseed_elements(GpuVec.from_numpy(pl, bad, FP)), lambda: coin.reseed_elements(bad, FP)):
            with pytest.raises(Exception, match=r"ms_coin_reseed_elements(_host)?: [dh]_elems holds an element that is not canonical.*row 1"):
                form()
            same_state(coin, ref)
    finally:
        pl.checked(False)
