"""The Poseidon public coin of the 252-bit field (ms_hades_coin_*, ministark_amd.coin.PoseidonCoin) against tests/hades_coin_ref.py: five
literal facts that neither the reference nor the kernels may misread, the seed forms, draws at the lane, wave and workgroup edges and at
the end of the u64 counter, the three reseeds at their padding edges, query positions, the proof-of-work search and its windows, the
refusals, the separation of the three coin families' handles, and checked mode.  The coin's record is read back (ms_hades_coin_read)
and compared with the reference after every step, not only what a step returns."""
import ctypes
import functools

import numpy as np
import pytest

from tests import backends, hades_coin_ref, poseidon_ref as pos
from ministark_amd import GOLDILOCKS_FP as GFP, GOLDILOCKS_FQ3 as GFQ3, STARK252_FP as F, GpuVec, Matrix, MerkleTree
from ministark_amd.api import F252_P as p, f252_from_mont_limbs, f252_to_mont_limbs

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
INVALID, UNSUPPORTED = -1, -2
MASK64 = (1 << 64) - 1

# the issue's five facts, as literals
FIRST_DRAW_OF_3 = 0x2ce6bb746235d2c43f8fd8ba3b6c9162cc0dd9f10afe408c73454151af510f5
DIGEST_3_THEN_5 = 0x12140abec1c89247c1bca9c94d4a3d016b8bcc20f83f648bc5d2ae38387890a
DIGEST_3_THEN_789 = 0x7bfc406d2b608cf22291e62d4c6357bb05f049e39802cbbb3adc9edd00219a5
GRIND_SEED, GRIND_NONCE = 3, 12158
GRIND_HIT = 0x4c72c56e8ce874c65eb456f6aac52cb5b3a7b78e9d7e54221cfb10f88640000


def pair(kind, seed=3):
    from ministark_amd.coin import PoseidonCoin
    return PoseidonCoin(backends.planner(kind), seed), hades_coin_ref.Coin(seed)


def same_state(coin, ref):
    assert coin.state() == ref.state()


def values(words):
    w = np.asarray(words, dtype=np.uint64).reshape(-1, 4)
    return [f252_from_mont_limbs(r) for r in w]


def mont(vals):
    return np.concatenate([f252_to_mont_limbs(v) for v in vals]).astype(np.uint64) if len(vals) else np.zeros(0, dtype=np.uint64)


def draw_both(coin, ref, count):
    got = values(coin.draw(F, count).to_numpy())
    assert got == ref.draw(count) and len(got) == count
    same_state(coin, ref)
    return got


def elements(count, rng):
    """canonical elements that include 0, 1 and p - 1"""
    return [[0, 1, p - 1][i] if i < 3 else int.from_bytes(rng.bytes(32), "little") % p for i in range(count)]


def test_the_reference_gives_the_five_facts():
    assert pos.permute(3, 0, 3)[0] == FIRST_DRAW_OF_3
    assert hades_coin_ref.Coin(3).draw(1) == [FIRST_DRAW_OF_3]
    ref = hades_coin_ref.Coin(3); ref.draw(2); ref.reseed_int(5)
    assert ref.state() == {"digest": DIGEST_3_THEN_5, "n_draws": 0} and pos.hash2(3, 5) == DIGEST_3_THEN_5
    ref = hades_coin_ref.Coin(3); ref.reseed_digest(5)
    assert ref.digest == DIGEST_3_THEN_5
    ref = hades_coin_ref.Coin(3); ref.reseed_elements([7, 8, 9])
    assert ref.digest == DIGEST_3_THEN_789 == pos.hash2(3, pos.hash_many([7, 8, 9])) and ref.permutations == 3
    assert pos.permute(3, GRIND_NONCE, 4)[0] == GRIND_HIT and GRIND_HIT % (1 << 18) == 0 and GRIND_HIT % (1 << 19) != 0
    assert hades_coin_ref.Coin(1).grind(12) == 2235 and hades_coin_ref.Coin(2).grind(12) == 2544
    assert 4096 < GRIND_NONCE <= 20480
    before = hades_coin_ref.Coin(3)
    before.reseed_elements([])
    assert before.state() == {"digest": 3, "n_draws": 0} and before.permutations == 0


@pytest.mark.parametrize("kind", KINDS)
def test_the_five_facts_on_the_device(kind):
    pl = backends.planner(kind)
    coin, _ = pair(kind)
    assert values(coin.draw(F, 1).to_numpy()) == [FIRST_DRAW_OF_3]
    assert coin.state() == {"digest": 3, "n_draws": 1}
    coin.reseed_int(5)
    assert coin.state() == {"digest": DIGEST_3_THEN_5, "n_draws": 0}
    coin, _ = pair(kind)
    coin.reseed_digest(GpuVec.from_numpy(pl, mont([5]), F).ptr)
    assert coin.state() == {"digest": DIGEST_3_THEN_5, "n_draws": 0}
    coin, _ = pair(kind)
    coin.reseed_elements(GpuVec.from_numpy(pl, mont([7, 8, 9]), F))
    assert coin.state() == {"digest": DIGEST_3_THEN_789, "n_draws": 0}
    coin, _ = pair(kind)
    for bits in range(12, 19):
        assert coin.grind(bits) == GRIND_NONCE, bits
    assert coin.state() == {"digest": 3, "n_draws": 0}
    assert pair(kind, 1)[0].grind(12) == 2235 and pair(kind, 2)[0].grind(12) == 2544           # inside the first window


@pytest.mark.parametrize("kind", KINDS)
def test_create_and_seed_forms(kind):
    from ministark_amd.coin import PoseidonCoin, poseidon_seed
    pl = backends.planner(kind)
    for seed in (0, 1, p - 1):
        coin, ref = pair(kind, seed)
        same_state(coin, ref)
        assert coin.state() == {"digest": seed, "n_draws": 0}
        as_bytes = PoseidonCoin(pl, seed.to_bytes(32, "little"))
        same_state(as_bytes, ref)
        draw_both(coin, ref, 1)
    assert poseidon_seed(bytes([7]) + bytes(31)) == 7
    for bad in (p, (1 << 256) - 1, -1, bytes(31), b"\xff" * 32, p.to_bytes(32, "little")):
        with pytest.raises(ValueError):
            PoseidonCoin(pl, bad)
    handle = ctypes.c_void_p()
    for bad in (p, (1 << 256) - 1):
        words = (ctypes.c_uint64 * 4)(*[(bad >> (64 * k)) & MASK64 for k in range(4)])
        assert pl.lib.ms_hades_coin_create(pl.handle, words, ctypes.byref(handle)) == INVALID and not handle.value


@pytest.mark.parametrize("kind", KINDS)
def test_draws_at_the_lane_wave_and_workgroup_edges(kind):
    total = 0
    coin, ref = pair(kind, 11)
    for count in (1, 2, 3, 64, 65, 257):                                      # 257: two workgroups, n_draws advanced by the trailing launch
        got = draw_both(coin, ref, count)
        total += count
        assert all(v < p for v in got) and coin.state()["n_draws"] == total
    draw_both(coin, ref, 256)                                                  # exactly one workgroup
    fresh, fref = pair(kind, 11)
    assert draw_both(fresh, fref, 3) == hades_coin_ref.Coin(11).draw(3)       # the same coin draws the same elements again


@pytest.mark.parametrize("kind", KINDS)
def test_draws_at_the_end_of_the_counter(kind):
    pl = backends.planner(kind)
    coin, ref = pair(kind)
    coin.set_state(3, (1 << 64) - 2)
    ref.n_draws = (1 << 64) - 2
    same_state(coin, ref)
    buf = GpuVec(pl, 3, F)
    assert pl.lib.ms_hades_coin_draw(pl.handle, coin.ptr, F, 3, buf.ptr) == INVALID           # counter 2^64 does not exist
    assert b"counter" in pl.lib.ms_last_error()
    n, qpos = ctypes.c_size_t(0), (ctypes.c_uint64 * 4)()
    assert pl.lib.ms_hades_coin_draw_queries(pl.handle, coin.ptr, 3, 16, qpos, ctypes.byref(n)) == INVALID
    same_state(coin, ref)
    got = values(coin.draw(F, 2).to_numpy())                                   # counters 2^64 - 2 and 2^64 - 1
    assert got == [pos.permute(3, (1 << 64) - 2, 3)[0], pos.permute(3, (1 << 64) - 1, 3)[0]] == ref.draw(2)
    same_state(coin, ref)


@pytest.mark.parametrize("kind", KINDS)
def test_reseed_elements_at_the_padding_edges(kind):
    from ministark_amd.coin import PoseidonCoin
    pl = backends.planner(kind)
    rng = np.random.default_rng(5)
    coin, ref = pair(kind)
    for count in (0, 1, 2, 3, 16):                                             # odd: the 1 completes the last pair; even: the 1 and a 0 open a new one
        elems = elements(count, rng)
        draw_both(coin, ref, 3)                                                # leave n_draws at 3: the reseed must reset it
        before, perms = coin.state(), ref.permutations
        if count:
            coin.reseed_elements(GpuVec.from_numpy(pl, mont(elems), F))
        else:
            assert pl.lib.ms_hades_coin_reseed_elements(pl.handle, coin.ptr, F, None, 0) == 0
        ref.reseed_elements(elems)
        same_state(coin, ref)
        assert ref.permutations - perms == (0 if count == 0 else count // 2 + 2)
        if count == 0:
            assert coin.state() == before and before["n_draws"] == 3          # not even n_draws changes
        host = PoseidonCoin(pl, 3)
        host.set_state(before["digest"], before["n_draws"])
        host.reseed_elements(mont(elems), F)                                   # the host form gives the same state
        same_state(host, ref)


@functools.lru_cache(maxsize=None)
def _tree(n):
    """(Montgomery columns, the reference's root) of an n-leaf Poseidon tree over 2 columns: computed once"""
    rng = np.random.default_rng(100 + n)
    cols = [[int.from_bytes(rng.bytes(32), "little") % p for _ in range(n)] for _ in range(2)]
    root = pos.merkle_nodes([pos.hash_many(r) for r in zip(*cols)])[1]
    return [mont(c) for c in cols], root


@pytest.mark.parametrize("n", [4, 1 << 10])
@pytest.mark.parametrize("kind", KINDS)
def test_reseed_digest_takes_the_root_where_the_tree_left_it(kind, n):
    pl = backends.planner(kind)
    cols, root = _tree(n)
    tree = MerkleTree.from_matrix(Matrix.from_numpy(pl, list(cols), F), hash="poseidon252")
    coin, ref = pair(kind)
    draw_both(coin, ref, 2)
    coin.reseed_digest(tree.root_ptr())
    ref.reseed_digest(root)
    same_state(coin, ref)
    assert ref.digest == pos.hash2(3, root)
    draw_both(coin, ref, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_reseed_int(kind):
    coin, ref = pair(kind)
    for v in (0, 1, 1 << 32, (1 << 64) - 1):
        draw_both(coin, ref, 1)
        coin.reseed_int(v)
        ref.reseed_int(v)
        same_state(coin, ref)
    # the domain tag: absorbing v is not what draw number v published
    assert pos.permute(3, 5, 2)[0] != pos.permute(3, 5, 3)[0]


@pytest.mark.parametrize("kind", KINDS)
def test_draw_queries(kind):
    pl = backends.planner(kind)
    coin, ref = pair(kind)
    drawn = 0
    for max_n, size in ((4, 1), (8, 2), (64, 16), (32, 1 << 20), (32, 1 << 32)):
        got, want = coin.draw_queries(max_n, size), ref.draw_queries(max_n, size)
        drawn += max_n
        assert got == want and all(q < size for q in got) and got == sorted(set(got))
        same_state(coin, ref)
        assert coin.state()["n_draws"] == drawn
        if (max_n, size) == (64, 16):
            assert len(got) <= 16 < max_n                                      # 64 samples over 16 positions: deduplicated
        if size == 1:
            assert got == [0]
    assert coin.draw_queries(0, 16) == []
    same_state(coin, ref)
    qpos, n = (ctypes.c_uint64 * 8)(), ctypes.c_size_t(0)
    for bad in (0, 3, 1 << 33):
        assert pl.lib.ms_hades_coin_draw_queries(pl.handle, coin.ptr, 4, bad, qpos, ctypes.byref(n)) == INVALID
        assert b"power of two" in pl.lib.ms_last_error()
    same_state(coin, ref)


@functools.lru_cache(maxsize=None)
def _ref_grind(seed, bits, max_nonce):
    """the reference's linear scan: run once, shared by the backends"""
    return hades_coin_ref.Coin(seed).grind(bits, max_nonce)


@pytest.mark.parametrize("kind", KINDS)
def test_grind_against_the_linear_search(kind):
    pl = backends.planner(kind)
    coin, ref = pair(kind, 7)
    draw_both(coin, ref, 2)
    assert coin.grind(0) == 1
    nonce = coin.grind(8)
    want = _ref_grind(7, 8, 1 << 14)
    print(f"bits 8: nonce {nonce}, reference {want}")
    assert nonce == want and nonce >= 1
    same_state(coin, ref)                                                      # grinding neither reseeds nor draws
    out = ctypes.c_uint64(0)
    assert pl.lib.ms_hades_coin_pow_grind(pl.handle, coin.ptr, 64, 1 << 20, ctypes.byref(out)) == INVALID
    assert pl.lib.ms_hades_coin_pow_grind(pl.handle, coin.ptr, 63, 1 << 10, ctypes.byref(out)) == INVALID   # accepted bits, nothing found
    same_state(coin, ref)
    coin.reseed_int(nonce)
    ref.reseed_int(nonce)
    same_state(coin, ref)
    assert coin.state()["digest"] != pos.permute(7, nonce, 4)[0]              # the digest after the reseed is another permutation's output


@pytest.mark.parametrize("kind", KINDS)
def test_grind_second_window(kind):
    pl = backends.planner(kind)
    coin, ref = pair(kind, GRIND_SEED)
    assert 4096 < GRIND_NONCE <= 20480
    assert _ref_grind(GRIND_SEED, 12, GRIND_NONCE) == GRIND_NONCE             # the reference's scan: nothing below it, and it is accepted
    assert coin.grind(12) == GRIND_NONCE
    same_state(coin, ref)
    out = ctypes.c_uint64(0)
    assert pl.lib.ms_hades_coin_pow_grind(pl.handle, coin.ptr, 12, GRIND_NONCE - 1, ctypes.byref(out)) == INVALID
    assert pl.lib.ms_hades_coin_pow_grind(pl.handle, coin.ptr, 12, GRIND_NONCE, ctypes.byref(out)) == 0 and out.value == GRIND_NONCE
    same_state(coin, ref)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_the_state_alone(kind):
    from ministark_amd._lib import HadesCoinState
    pl = backends.planner(kind)
    L, h = pl.lib, pl.handle
    coin, ref = pair(kind)
    draw_both(coin, ref, 1)
    buf = GpuVec.from_numpy(pl, mont([1, 2, 3, 4]), F)
    gbuf = GpuVec(pl, 16, GFP)
    n, out, handle = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_void_p()
    qpos = (ctypes.c_uint64 * 4)()
    seed = (ctypes.c_uint64 * 4)(3, 0, 0, 0)

    def record(digest=None, pad=None):
        st = HadesCoinState()
        if digest is not None:
            for k in range(4):
                st.digest[k] = (digest >> (64 * k)) & MASK64
        if pad is not None:
            st.pad[pad] = 1
        return ctypes.byref(st)

    refused = [
        L.ms_hades_coin_create(h, None, ctypes.byref(handle)),
        L.ms_hades_coin_create(h, seed, None),
        L.ms_hades_coin_read(h, coin.ptr, None),
        L.ms_hades_coin_read(h, None, record()),
        L.ms_hades_coin_write(h, coin.ptr, None),
        L.ms_hades_coin_write(h, coin.ptr, record(digest=p)),                                         # Montgomery words = p
        L.ms_hades_coin_write(h, coin.ptr, record(digest=(1 << 256) - 1)),
        L.ms_hades_coin_write(h, coin.ptr, record(pad=0)),
        L.ms_hades_coin_write(h, coin.ptr, record(pad=3)),
        L.ms_hades_coin_reseed_digest(h, coin.ptr, None),
        L.ms_hades_coin_reseed_digest(h, None, buf.ptr),
        L.ms_hades_coin_reseed_digest(h, buf.ptr, buf.ptr),                                           # not a coin of this context
        L.ms_hades_coin_reseed_int(h, None, 1),
        L.ms_hades_coin_reseed_int(h, buf.ptr, 1),
        L.ms_hades_coin_reseed_elements(h, coin.ptr, 7, buf.ptr, 1),                                  # unknown field
        L.ms_hades_coin_reseed_elements(h, coin.ptr, F, None, 1),
        L.ms_hades_coin_reseed_elements_host(h, coin.ptr, 7, buf.ptr, 1),
        L.ms_hades_coin_reseed_elements_host(h, coin.ptr, F, None, 1),
        L.ms_hades_coin_draw(h, coin.ptr, 7, 1, buf.ptr),
        L.ms_hades_coin_draw(h, coin.ptr, F, 1, None),
        L.ms_hades_coin_draw(h, coin.ptr, F, 1, coin.ptr),                                            # into its own state
        L.ms_hades_coin_draw_queries(h, coin.ptr, 4, 16, None, ctypes.byref(n)),
        L.ms_hades_coin_draw_queries(h, coin.ptr, 4, 16, qpos, None),
        L.ms_hades_coin_pow_grind(h, coin.ptr, 64, 1 << 20, ctypes.byref(out)),                       # bits > 63
        L.ms_hades_coin_pow_grind(h, coin.ptr, 8, 1 << 20, None),
        L.ms_hades_coin_destroy(h, buf.ptr),
    ]
    assert refused == [INVALID] * len(refused)
    unsupported = [
        L.ms_hades_coin_draw(h, coin.ptr, GFP, 1, gbuf.ptr),
        L.ms_hades_coin_draw(h, coin.ptr, GFQ3, 1, gbuf.ptr),
        L.ms_hades_coin_reseed_elements(h, coin.ptr, GFP, gbuf.ptr, 1),
        L.ms_hades_coin_reseed_elements(h, coin.ptr, GFQ3, gbuf.ptr, 1),
        L.ms_hades_coin_reseed_elements_host(h, coin.ptr, GFP, gbuf.ptr, 1),
        L.ms_hades_coin_reseed_elements_host(h, coin.ptr, GFQ3, gbuf.ptr, 1),
    ]
    assert unsupported == [UNSUPPORTED] * len(unsupported)
    same_state(coin, ref)
    assert L.ms_hades_coin_destroy(h, None) == 0
    assert L.ms_hades_coin_write(h, coin.ptr, record(digest=p - 1)) == 0                              # the accepted edge: Montgomery words p - 1
    assert coin.state() == {"digest": (p - 1) * pow(1 << 256, -1, p) % p, "n_draws": 0}


@pytest.mark.parametrize("kind", KINDS)
def test_the_three_coin_families_refuse_each_others_handles(kind):
    from ministark_amd._lib import CoinState, HadesCoinState, RpoCoinState
    from ministark_amd.coin import PublicCoin, RpoCoin
    pl = backends.planner(kind)
    L, h = pl.lib, pl.handle
    coin, ref = pair(kind)
    byte_coin = PublicCoin(pl, bytes(range(32)), "sha256")
    rpo_coin = RpoCoin(pl, [1, 2, 3, 4])
    before_byte, before_rpo = byte_coin.state(), rpo_coin.state()
    buf = GpuVec.from_numpy(pl, mont([1, 2]), F)
    n, out, qpos = ctypes.c_size_t(0), ctypes.c_uint64(0), (ctypes.c_uint64 * 4)()
    crossed = []
    for other in (byte_coin, rpo_coin):                                        # their handles, our entry points
        crossed += [
            L.ms_hades_coin_read(h, other.ptr, ctypes.byref(HadesCoinState())),
            L.ms_hades_coin_write(h, other.ptr, ctypes.byref(HadesCoinState())),
            L.ms_hades_coin_reseed_int(h, other.ptr, 1),
            L.ms_hades_coin_reseed_digest(h, other.ptr, buf.ptr),
            L.ms_hades_coin_reseed_elements(h, other.ptr, F, buf.ptr, 1),
            L.ms_hades_coin_draw(h, other.ptr, F, 1, buf.ptr),
            L.ms_hades_coin_draw_queries(h, other.ptr, 4, 16, qpos, ctypes.byref(n)),
            L.ms_hades_coin_pow_grind(h, other.ptr, 4, 1 << 20, ctypes.byref(out)),
            L.ms_hades_coin_destroy(h, other.ptr),
        ]
    crossed += [                                                               # our handle, their entry points
        L.ms_coin_read(h, coin.ptr, ctypes.byref(CoinState())),
        L.ms_coin_reseed_int(h, coin.ptr, 1),
        L.ms_coin_reseed_digest(h, coin.ptr, buf.ptr),
        L.ms_coin_draw(h, coin.ptr, F, 1, buf.ptr),
        L.ms_coin_draw_queries(h, coin.ptr, 4, 16, qpos, ctypes.byref(n)),
        L.ms_coin_pow_grind(h, coin.ptr, 4, 1 << 20, ctypes.byref(out)),
        L.ms_coin_destroy(h, coin.ptr),
        L.ms_rpo_coin_read(h, coin.ptr, ctypes.byref(RpoCoinState())),
        L.ms_rpo_coin_reseed_int(h, coin.ptr, 1),
        L.ms_rpo_coin_reseed_digest(h, coin.ptr, buf.ptr),
        L.ms_rpo_coin_draw(h, coin.ptr, GFP, 1, buf.ptr),
        L.ms_rpo_coin_draw_queries(h, coin.ptr, 4, 16, qpos, ctypes.byref(n)),
        L.ms_rpo_coin_pow_grind(h, coin.ptr, 4, 1 << 20, ctypes.byref(out)),
        L.ms_rpo_coin_destroy(h, coin.ptr),
    ]
    assert crossed == [INVALID] * len(crossed)
    same_state(coin, ref)
    assert byte_coin.state() == before_byte and rpo_coin.state() == before_rpo
    with pytest.raises(ValueError, match="unknown coin hash"):
        PublicCoin(pl, bytes(32), "poseidon252")                               # ms_coin_create's hash ids are what they were


@pytest.mark.parametrize("kind", KINDS)
def test_checked_mode_scans_what_the_reseeds_absorb(kind):
    pl = backends.planner(kind)
    coin, ref = pair(kind)
    bad = np.concatenate([f252_to_mont_limbs(5), np.array([(p >> (64 * k)) & MASK64 for k in range(4)], dtype=np.uint64), f252_to_mont_limbs(6)])
    pl.checked(True)
    try:
        for form in (lambda: coin.reseed_elements(GpuVec.from_numpy(pl, bad, F)), lambda: coin.reseed_elements(bad, F)):
            with pytest.raises(Exception, match=r"ms_hades_coin_reseed_elements(_host)?: [dh]_elems holds an element that is not canonical.*row 1"):
                form()
            same_state(coin, ref)
        with pytest.raises(Exception, match=r"ms_hades_coin_reseed_digest: d_digest holds an element that is not canonical.*row 0"):
            coin.reseed_digest(GpuVec.from_numpy(pl, bad[4:8], F).ptr)
        same_state(coin, ref)
        coin.reseed_digest(GpuVec.from_numpy(pl, bad[:4], F).ptr)              # canonical input passes in checked mode
        ref.reseed_digest(5)
        same_state(coin, ref)
    finally:
        pl.checked(False)
