"""The device-resident public coin with H = BLAKE3 (id 6, hash="blake3_256") against tests/blake3_ref.Coin: the scenarios of
tests/test_keccak_coin.py -- the reseeds, draws in all three fields (a draw that straddles a digest, the rejection path of the 252-bit
sampler), reseed_elements with 0, 1, 2 and 65 elements, query positions, the proof-of-work search from the device seed, state read
and write.  The coin's state is read back and compared after every step.  Ids 2, 5 and -1 stay refused.

tests/coin_ref.py cannot take a hash function, so tests/blake3_ref.Coin restates every rule that hashes over the helper's blake3()."""
import ctypes

import numpy as np
import pytest

from tests import backends, blake3_ref
from tests.test_public_coin import SEED, draw_both, elements, same_state
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as FP252, GpuVec, grind_proof_of_work
from ministark_amd.api import F252_P, GL_P
from ministark_amd.coin import HASH_IDS, PublicCoin

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
HASH = "blake3_256"


def pair(kind, seed=SEED):
    return PublicCoin(backends.planner(kind), seed, HASH), blake3_ref.Coin(seed)


def test_id_and_the_coin_words_come_from_the_helper():
    assert HASH_IDS[HASH] == 6 and 2 not in HASH_IDS.values() and 5 not in HASH_IDS.values() and "blake3" not in HASH_IDS
    ref = blake3_ref.Coin(SEED)
    d = blake3_ref.blake3(SEED + (1).to_bytes(8, "big"))
    assert [ref.word() for _ in range(4)] == [int.from_bytes(d[24 - 8 * k: 32 - 8 * k], "little") for k in range(4)]


@pytest.mark.parametrize("kind", KINDS)
def test_goldilocks_draws_cross_digest_boundaries(kind):
    for count in (1, 4, 5, 9):                                     # a digest is 4 words: whole digests, and one word past a boundary
        coin, ref = pair(kind)
        same_state(coin, ref)
        words = draw_both(coin, ref, FP, count)
        assert all(w < GL_P for w in words)
    draw_both(coin, ref, FP, 2)                                    # 9 + 2: continues inside the third digest


@pytest.mark.parametrize("kind", KINDS)
def test_fq3_draws_take_c0_c1_c2_in_order(kind):
    coin, ref = pair(kind)
    for count in (1, 2, 3):                                        # words 0-2, then 3-8: the second draw straddles a digest
        assert len(draw_both(coin, ref, FQ3, count)) == 3 * count


@pytest.mark.parametrize("kind", KINDS)
def test_fp252_draws_reject_about_half_the_samples(kind):
    for seed in (SEED, bytes(31) + b"\x07"):
        coin, ref = pair(kind, seed)
        limbs = draw_both(coin, ref, FP252, 8)
        assert ref.rejections >= 1 and ref.first_try >= 1         # both branches of the sampler were taken
        for i in range(8):
            assert sum(v << (64 * k) for k, v in enumerate(limbs[4 * i: 4 * i + 4])) < F252_P


@pytest.mark.parametrize("kind", KINDS)
def test_goldilocks_rejection_branch_and_state_write(kind):
    le = lambda v: int(v).to_bytes(8, "little")                    # noqa: E731
    for first, second, want in (((1 << 64) - 1, 12345, 12345), (GL_P, 777, 777), (GL_P - 1, 777, GL_P - 1)):
        coin, ref = pair(kind)
        unread = le(second) + le(first)                            # consumed from the end: `first` comes out first
        coin.set_state(SEED, 3, unread)
        ref.seed, ref.counter, ref.unread = SEED, 3, unread
        same_state(coin, ref)
        assert draw_both(coin, ref, FP, 1) == [want]
        assert ref.rejections == (0 if want == first else 1)


@pytest.mark.parametrize("kind", KINDS)
def test_reseeds(kind):
    pl = backends.planner(kind)
    rng = np.random.default_rng(5)
    coin, ref = pair(kind)
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
            host, _ = pair(kind)
            host.set_state(before["seed"], before["counter"], before["unread"])
            host.reseed_elements(words, field)                     # the host form gives the same state
            same_state(host, ref)


@pytest.mark.parametrize("kind", KINDS)
def test_interleaved_script(kind):
    pl = backends.planner(kind)
    coin, ref = pair(kind, b"\xa5" * 32)
    draw_both(coin, ref, FP, 3)
    root = bytes(range(100, 132))
    coin.reseed_digest(GpuVec.from_numpy(pl, np.frombuffer(root, dtype=np.uint64)).ptr)
    ref.reseed_digest(root)
    draw_both(coin, ref, FP252, 1)
    coin.reseed_int(99)
    ref.reseed_int(99)
    draw_both(coin, ref, FP, 6)
    draw_both(coin, ref, FQ3, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_draw_queries(kind):
    coin, ref = pair(kind)
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


@pytest.mark.parametrize("kind", KINDS)
def test_pow_grind_uses_the_seed_on_the_device(kind):
    pl = backends.planner(kind)
    coin, ref = pair(kind)
    coin.reseed_int(4)
    ref.reseed_int(4)
    for bits in (8, 12):
        nonce = coin.grind(bits)
        assert nonce == grind_proof_of_work(pl, coin.state()["seed"], bits, hash=HASH)
        assert nonce == ref.grind(bits)
        same_state(coin, ref)                                      # grinding does not reseed


@pytest.mark.parametrize("kind", KINDS)
def test_ids_2_and_5_are_still_refused_and_6_is_accepted(kind):
    pl = backends.planner(kind)
    L, h = pl.lib, pl.handle
    handle = ctypes.c_void_p()
    seed = ctypes.create_string_buffer(SEED, 32)
    for bad in (2, 5, -1, 7):
        assert L.ms_coin_create(h, bad, seed, ctypes.byref(handle)) == -1
        assert b"unknown hash id" in L.ms_last_error()
    for good in (0, 1, 3, 4, 6):
        assert L.ms_coin_create(h, good, seed, ctypes.byref(handle)) == 0
        assert L.ms_coin_destroy(h, handle) == 0
    with pytest.raises(ValueError, match="unknown coin hash"):
        PublicCoin(pl, SEED, "blake3")
