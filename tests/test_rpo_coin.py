"""The RPO-256 public coin (ms_rpo_coin_*, ministark_amd.coin.RpoCoin) against tests/rpo_coin_ref.py: draws on, before and after a refill
of the rate, the three reseeds at their block edges, query positions, the proof-of-work search and its windows, the refusals, the
separation from the byte coin's handles, and the ABI.  The coin's record is read back (ms_rpo_coin_read) and compared with the reference
after every step, not only what a step returns."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

from tests import backends, rpo_coin_ref
from tests.test_rust_shim import _expect
from oracle.pyref import rpo as pyrpo
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as FP252, GpuVec, Matrix, MerkleTree
from ministark_amd.api import GL_P, gl_from_mont, gl_to_mont

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
SEED = [1, 2, 3, 4]
# rpo_coin_ref.Coin(GRIND_SEED).grind(12) == GRIND_NONCE: past the first window of mscommit::grind_windows (nonces 1..4096), inside the
# second (4097..20480).  Picked with the reference; test_grind_second_window re-checks it by the reference's own linear scan.
GRIND_SEED = [12, 0, 0, 0]
GRIND_NONCE = 4969
INVALID, UNSUPPORTED = -1, -2


def pair(kind, seed=SEED):
    from ministark_amd.coin import RpoCoin
    return RpoCoin(backends.planner(kind), seed), rpo_coin_ref.Coin(seed)


def same_state(coin, ref):
    assert coin.state() == ref.state()


def draw_both(coin, ref, field, count):
    got = [gl_from_mont(int(v)) for v in coin.draw(field, count).to_numpy()]
    assert got == ref.draw(count * (3 if field == FQ3 else 1))
    same_state(coin, ref)
    return got


def elements(nwords, rng):
    """canonical words that include 0, 1 and p - 1"""
    return [[0, 1, GL_P - 1][i] if i < 3 else int(rng.integers(0, GL_P, dtype=np.uint64)) for i in range(nwords)]


def mont(words):
    return np.array([gl_to_mont(w) for w in words], dtype=np.uint64)


def test_the_reference_follows_the_rules_by_hand():
    ref = rpo_coin_ref.Coin(SEED)
    s0 = pyrpo.permute([0, 0, 0, 0, 1, 2, 3, 4, 0, 0, 0, 0])
    assert ref.state() == {"s": s0, "pos": 4}
    assert ref.draw(8) == s0[4:12] and ref.pos == 12
    s1 = pyrpo.permute(s0)
    assert ref.draw(1) == [s1[4]] and ref.pos == 5                              # the ninth word comes from the next permutation
    ref.reseed_int((7 << 32) | 9)
    t = list(s1); t[4] = (t[4] + 9) % GL_P; t[5] = (t[5] + 7) % GL_P
    assert ref.state() == {"s": pyrpo.permute(t), "pos": 4}
    before = ref.copy()
    ref.reseed_elements([5] * 8)                                               # a full block: the 1 opens a second one
    t = list(before.s)
    for j in range(8):
        t[4 + j] = (t[4 + j] + 5) % GL_P
    t = pyrpo.permute(t); t[4] = (t[4] + 1) % GL_P
    assert ref.s == pyrpo.permute(t) and ref.permutations == before.permutations + 2


@pytest.mark.parametrize("kind", KINDS)
def test_create_and_seed_forms(kind):
    from ministark_amd.coin import RpoCoin
    coin, ref = pair(kind)
    same_state(coin, ref)
    as_bytes = RpoCoin(backends.planner(kind), b"".join(int(v).to_bytes(8, "little") for v in SEED))
    same_state(as_bytes, ref)
    edge = [0, 1, GL_P - 1, 1 << 63]
    coin, ref = pair(kind, edge)
    same_state(coin, ref)
    for bad in ([1, 2, 3], [1, 2, 3, GL_P], bytes(31), b"\xff" * 32):
        with pytest.raises(ValueError):
            RpoCoin(backends.planner(kind), bad)


@pytest.mark.parametrize("kind", KINDS)
def test_fp_draws_on_before_and_after_a_refill(kind):
    for count in (1, 7, 8, 9, 16, 17):                                         # the rate holds 8 words
        coin, ref = pair(kind)
        words = draw_both(coin, ref, FP, count)
        assert all(w < GL_P for w in words) and len(words) == count
    draw_both(coin, ref, FP, 2)                                                # 17 + 2: continues inside the third block
    draw_both(coin, ref, FP, 5)                                                # ... and ends exactly on its last word (pos = 12)
    assert ref.pos == 12
    draw_both(coin, ref, FP, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_fq3_draws_take_three_consecutive_words(kind):
    for count in (1, 3, 8):                                                    # 3 words; 9 words straddle a refill; 24 = three blocks
        coin, ref = pair(kind)
        assert len(draw_both(coin, ref, FQ3, count)) == 3 * count
    draw_both(coin, ref, FQ3, 1)
    draw_both(coin, ref, FP, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_reseed_elements_at_the_block_edges(kind):
    from ministark_amd.coin import RpoCoin
    pl = backends.planner(kind)
    rng = np.random.default_rng(5)
    coin, ref = pair(kind)
    for field, counts in ((FP, (0, 1, 7, 8, 9, 63, 64, 65)), (FQ3, (1, 3, 8))):   # 7: the pad fills the block; 8: it opens a new one
        V = 3 if field == FQ3 else 1
        for count in counts:
            words = elements(count * V, rng)
            draw_both(coin, ref, FP, 3)                                        # leave pos in the middle: the reseed must reset it
            before, perms = coin.state(), ref.permutations
            coin.reseed_elements(GpuVec.from_numpy(pl, mont(words), field))
            ref.reseed_elements(words)
            same_state(coin, ref)
            assert ref.permutations - perms == (0 if count == 0 else count * V // 8 + 1)
            if count == 0:
                assert coin.state() == before and before["pos"] == 7           # not even pos changes
            host = RpoCoin(pl, SEED)
            host.set_state(before["s"], before["pos"])
            host.reseed_elements(mont(words), field)                           # the host form gives the same state
            same_state(host, ref)


@functools.lru_cache(maxsize=None)
def _tree_nodes(n):
    """(Montgomery columns, the reference's nodes) of an n-leaf RPO tree over 3 Fp columns: computed once"""
    rng = np.random.default_rng(100 + n)
    cols = [rng.integers(0, GL_P, size=n, dtype=np.uint64) for _ in range(3)]
    leaves = [pyrpo.hash_row([gl_from_mont(int(c[r])) for c in cols]) for r in range(n)]
    return cols, pyrpo.merkle_nodes(leaves)


@pytest.mark.parametrize("n", [4, 1 << 10])
@pytest.mark.parametrize("kind", KINDS)
def test_reseed_digest_takes_the_root_where_the_tree_left_it(kind, n):
    pl = backends.planner(kind)
    cols, nodes = _tree_nodes(n)
    tree = MerkleTree.from_matrix(Matrix.from_numpy(pl, list(cols), FP), hash="rpo256")
    coin, ref = pair(kind)
    draw_both(coin, ref, FP, 2)
    coin.reseed_digest(tree.root_ptr())
    ref.reseed_digest(nodes[1])
    same_state(coin, ref)
    draw_both(coin, ref, FQ3, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_reseed_int_splits_the_value_in_two_halves(kind):
    coin, ref = pair(kind)
    for v in (0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1):
        draw_both(coin, ref, FP, 1)
        coin.reseed_int(v)
        ref.reseed_int(v)
        same_state(coin, ref)


@pytest.mark.parametrize("kind", KINDS)
def test_draw_queries(kind):
    pl = backends.planner(kind)
    coin, ref = pair(kind)
    for max_n, size in ((4, 1), (8, 2), (16, 8), (32, 1 << 20), (32, 1 << 32)):
        got, want = coin.draw_queries(max_n, size), ref.draw_queries(max_n, size)
        assert got == want and all(p < size for p in got) and got == sorted(set(got))
        same_state(coin, ref)
    assert coin.draw_queries(4, 1) == [0] and ref.draw_queries(4, 1) == [0]
    assert len(coin.draw_queries(8, 2)) <= 2 and ref.draw_queries(8, 2) is not None     # max_n above the domain size
    same_state(coin, ref)
    assert coin.draw_queries(0, 16) == []
    same_state(coin, ref)
    pos, n = (ctypes.c_uint64 * 8)(), ctypes.c_size_t(0)
    for bad in (0, 3, 1 << 33):
        assert pl.lib.ms_rpo_coin_draw_queries(pl.handle, coin.ptr, 4, bad, pos, ctypes.byref(n)) == INVALID
        assert b"power of two" in pl.lib.ms_last_error()
    same_state(coin, ref)


@functools.lru_cache(maxsize=None)
def _ref_grind(seed, reseed, bits, max_nonce):
    """the reference's linear search from Coin(seed) [after reseed_int(reseed)]: scanned once, shared by the backends"""
    ref = rpo_coin_ref.Coin(seed)
    if reseed is not None:
        ref.reseed_int(reseed)
    return ref.grind(bits, max_nonce)


@pytest.mark.parametrize("kind", KINDS)
def test_grind_against_the_linear_search(kind):
    coin, ref = pair(kind)
    coin.reseed_int(3)                                                         # (the 12-bit nonce of this state is 3594: a short scan)
    ref.reseed_int(3)
    for bits in (0, 1, 8, 12):
        nonce = coin.grind(bits)
        want = _ref_grind(tuple(SEED), 3, bits, 1 << 14)
        print(f"bits {bits}: nonce {nonce}, reference {want}")
        assert nonce == want and nonce >= 1
        same_state(coin, ref)                                                  # grinding does not reseed
    assert coin.grind(0) == 1
    after, rafter = pair(kind)
    after.set_state(coin.state()["s"], coin.state()["pos"])
    rafter.s, rafter.pos = list(ref.s), ref.pos
    after.reseed_int(nonce)
    rafter.reseed_int(nonce)
    same_state(after, rafter)
    assert after.state()["s"][0] & 0xFFF == 0                                  # the state after the reseed IS the accepted t
    out = ctypes.c_uint64(0)
    pl = backends.planner(kind)
    assert pl.lib.ms_rpo_coin_pow_grind(pl.handle, coin.ptr, 64, 1 << 20, ctypes.byref(out)) == INVALID
    same_state(coin, ref)


@pytest.mark.parametrize("kind", KINDS)
def test_grind_second_window(kind):
    pl = backends.planner(kind)
    coin, ref = pair(kind, GRIND_SEED)
    assert 4096 < GRIND_NONCE <= 20480
    assert _ref_grind(tuple(GRIND_SEED), None, 12, GRIND_NONCE) == GRIND_NONCE                           # the reference's scan: nothing below it, and it is accepted
    assert coin.grind(12) == GRIND_NONCE
    same_state(coin, ref)
    out = ctypes.c_uint64(0)
    assert pl.lib.ms_rpo_coin_pow_grind(pl.handle, coin.ptr, 12, GRIND_NONCE - 1, ctypes.byref(out)) == INVALID
    assert pl.lib.ms_rpo_coin_pow_grind(pl.handle, coin.ptr, 12, GRIND_NONCE, ctypes.byref(out)) == 0 and out.value == GRIND_NONCE
    same_state(coin, ref)
    coin.reseed_int(GRIND_NONCE)
    ref.reseed_int(GRIND_NONCE)
    same_state(coin, ref)
    assert coin.state()["s"][0] & 0xFFF == 0


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_the_state_alone(kind):
    from ministark_amd._lib import RpoCoinState
    pl = backends.planner(kind)
    L, h = pl.lib, pl.handle
    coin, ref = pair(kind)
    draw_both(coin, ref, FP, 1)
    buf = GpuVec(pl, 16, FP)
    n, out, handle = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_void_p()
    pos = (ctypes.c_uint64 * 4)()
    seed = (ctypes.c_uint64 * 4)(1, 2, 3, 4)

    def record(pos=4, word=None, pad=None):
        st = RpoCoinState()
        st.pos = pos
        if word is not None:
            st.s[word] = GL_P
        if pad is not None:
            st.pad[pad] = 1
        return ctypes.byref(st)

    refused = [
        L.ms_rpo_coin_create(h, None, ctypes.byref(handle)),
        L.ms_rpo_coin_create(h, seed, None),
        L.ms_rpo_coin_create(h, (ctypes.c_uint64 * 4)(1, 2, GL_P, 4), ctypes.byref(handle)),          # a seed word = p
        L.ms_rpo_coin_read(h, coin.ptr, None),
        L.ms_rpo_coin_read(h, None, record()),
        L.ms_rpo_coin_write(h, coin.ptr, None),
        L.ms_rpo_coin_write(h, coin.ptr, record(pos=3)),
        L.ms_rpo_coin_write(h, coin.ptr, record(pos=13)),
        L.ms_rpo_coin_write(h, coin.ptr, record(word=0)),                                             # a word = p, capacity and rate
        L.ms_rpo_coin_write(h, coin.ptr, record(word=11)),
        L.ms_rpo_coin_write(h, coin.ptr, record(pad=0)),
        L.ms_rpo_coin_write(h, coin.ptr, record(pad=6)),
        L.ms_rpo_coin_reseed_digest(h, coin.ptr, None),
        L.ms_rpo_coin_reseed_digest(h, None, buf.ptr),
        L.ms_rpo_coin_reseed_digest(h, buf.ptr, buf.ptr),                                             # not a coin of this context
        L.ms_rpo_coin_reseed_int(h, None, 1),
        L.ms_rpo_coin_reseed_int(h, buf.ptr, 1),
        L.ms_rpo_coin_reseed_elements(h, coin.ptr, 7, buf.ptr, 1),                                    # unknown field
        L.ms_rpo_coin_reseed_elements(h, coin.ptr, FP, None, 1),
        L.ms_rpo_coin_reseed_elements_host(h, coin.ptr, 7, buf.ptr, 1),
        L.ms_rpo_coin_reseed_elements_host(h, coin.ptr, FP, None, 1),
        L.ms_rpo_coin_draw(h, coin.ptr, 7, 1, buf.ptr),
        L.ms_rpo_coin_draw(h, coin.ptr, FP, 1, None),
        L.ms_rpo_coin_draw(h, coin.ptr, FP, 1, coin.ptr),                                             # into its own state
        L.ms_rpo_coin_draw_queries(h, coin.ptr, 4, 16, None, ctypes.byref(n)),
        L.ms_rpo_coin_draw_queries(h, coin.ptr, 4, 16, pos, None),
        L.ms_rpo_coin_pow_grind(h, coin.ptr, 64, 1 << 20, ctypes.byref(out)),                         # bits > 63
        L.ms_rpo_coin_pow_grind(h, coin.ptr, 8, 1 << 20, None),
        L.ms_rpo_coin_destroy(h, buf.ptr),
    ]
    assert refused == [INVALID] * len(refused)
    unsupported = [
        L.ms_rpo_coin_draw(h, coin.ptr, FP252, 1, buf.ptr),
        L.ms_rpo_coin_reseed_elements(h, coin.ptr, FP252, buf.ptr, 1),
        L.ms_rpo_coin_reseed_elements_host(h, coin.ptr, FP252, buf.ptr, 1),
    ]
    assert unsupported == [UNSUPPORTED] * 3
    same_state(coin, ref)
    assert L.ms_rpo_coin_write(h, coin.ptr, record(pos=12)) == 0                                      # the accepted edges: pos 12, zero state
    assert coin.state() == {"s": [0] * 12, "pos": 12}


@pytest.mark.parametrize("kind", KINDS)
def test_the_two_coin_families_refuse_each_others_handles(kind):
    from ministark_amd._lib import CoinState, RpoCoinState
    from ministark_amd.coin import PublicCoin
    pl = backends.planner(kind)
    L, h = pl.lib, pl.handle
    coin, ref = pair(kind)
    byte_coin = PublicCoin(pl, bytes(range(32)), "sha256")
    before = byte_coin.state()
    buf = GpuVec(pl, 8, FP)
    n, out, pos = ctypes.c_size_t(0), ctypes.c_uint64(0), (ctypes.c_uint64 * 4)()
    crossed = [
        L.ms_rpo_coin_read(h, byte_coin.ptr, ctypes.byref(RpoCoinState())),
        L.ms_rpo_coin_reseed_int(h, byte_coin.ptr, 1),
        L.ms_rpo_coin_reseed_digest(h, byte_coin.ptr, buf.ptr),
        L.ms_rpo_coin_draw(h, byte_coin.ptr, FP, 1, buf.ptr),
        L.ms_rpo_coin_draw_queries(h, byte_coin.ptr, 4, 16, pos, ctypes.byref(n)),
        L.ms_rpo_coin_pow_grind(h, byte_coin.ptr, 4, 1 << 20, ctypes.byref(out)),
        L.ms_rpo_coin_destroy(h, byte_coin.ptr),
        L.ms_coin_read(h, coin.ptr, ctypes.byref(CoinState())),
        L.ms_coin_reseed_int(h, coin.ptr, 1),
        L.ms_coin_reseed_digest(h, coin.ptr, buf.ptr),
        L.ms_coin_draw(h, coin.ptr, FP, 1, buf.ptr),
        L.ms_coin_draw_queries(h, coin.ptr, 4, 16, pos, ctypes.byref(n)),
        L.ms_coin_pow_grind(h, coin.ptr, 4, 1 << 20, ctypes.byref(out)),
        L.ms_coin_destroy(h, coin.ptr),
    ]
    assert crossed == [INVALID] * len(crossed)
    same_state(coin, ref)
    assert byte_coin.state() == before


@pytest.mark.parametrize("kind", KINDS)
def test_checked_mode_scans_what_the_reseeds_absorb(kind):
    pl = backends.planner(kind)
    coin, ref = pair(kind)
    bad = np.array([gl_to_mont(5), GL_P + 1, gl_to_mont(6), 0], dtype=np.uint64)
    pl.checked(True)
    try:
        for form in (lambda: coin.reseed_elements(GpuVec.from_numpy(pl, bad, FP)), lambda: coin.reseed_elements(bad, FP)):
            with pytest.raises(Exception, match=r"ms_rpo_coin_reseed_elements(_host)?: [dh]_elems holds an element that is not canonical.*row 1"):
                form()
            same_state(coin, ref)
        with pytest.raises(Exception, match=r"ms_rpo_coin_reseed_digest: d_digest4 holds an element that is not canonical.*row 1"):
            coin.reseed_digest(GpuVec.from_numpy(pl, bad, FP).ptr)
        same_state(coin, ref)
    finally:
        pl.checked(False)


# ---- ABI: the header, the library, _lib.Lib.rpo_coin_sigs and rust/gpu/src/hip/sys_rpo_coin.rs agree

HEADER = os.path.join(ROOT, "include", "ministark_hip_rpo_coin.h")
NAMES = sorted("ms_rpo_coin_" + n for n in ("create", "destroy", "read", "write", "reseed_digest", "reseed_int", "reseed_elements",
                                             "reseed_elements_host", "draw", "draw_queries", "pow_grind"))
OLDER = ("ministark_hip.h", "ministark_hip_transcript.h", "ministark_hip_keccak.h", "ministark_hip_ext.h", "ministark_hip_logup.h")


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    return {m.group(1): [p.strip() for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\b(ms_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)}


def test_header_library_and_ctypes_binding_agree():
    from ministark_amd import _lib, build
    protos = _prototypes()
    assert sorted(protos) == NAMES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert not [n for n in NAMES if not hasattr(lib, n)]
    L = _lib.Lib()
    assert sorted(L.rpo_coin_sigs) == NAMES
    assert not set(NAMES) & (set(L.sigs) | set(L.transcript_sigs) | set(L.keccak_sigs) | set(L.ext_sigs) | set(L.logup_sigs))
    for name, params in protos.items():
        assert len(L.rpo_coin_sigs[name][1]) == len(params), name
        assert getattr(L, name).argtypes == L.rpo_coin_sigs[name][1]
        twin = L.transcript_sigs[name.replace("ms_rpo_coin_", "ms_coin_")]          # each the twin of its namesake, minus `hash`
        want = [a for k, a in enumerate(twin[1]) if not (name.endswith("_create") and k == 1)]
        assert L.rpo_coin_sigs[name] == (twin[0], want), name
    for older in OLDER:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", older)).read(), flags=re.S)
        assert "rpo_coin" not in text.lower(), older
    text = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert '#include "ministark_hip_transcript.h"' in text
    body = re.search(r"typedef struct ms_rpo_coin_state \{(.*?)\} ms_rpo_coin_state;", text).group(1)
    assert [tuple(m.split()) for m in body.split(";") if m.strip()] == [("uint64_t", "s[12]"), ("uint32_t", "pos"), ("uint32_t", "pad[7]")]
    assert ctypes.sizeof(_lib.RpoCoinState) == 128 and ctypes.alignment(_lib.RpoCoinState) == 8
    assert [(n, ctypes.sizeof(t)) for n, t in _lib.RpoCoinState._fields_] == [("s", 96), ("pos", 4), ("pad", 28)]
    assert _lib.RpoCoinState.pos.offset == 96 and _lib.RpoCoinState.pad.offset == 100
    kernels = open(os.path.join(ROOT, "ministark_amd", "csrc", "rpo_coin_kernels.h")).read()
    assert "static_assert(sizeof(State) == 128" in kernels
    assert "ms_rpo_coin.cpp" in build.SOURCES


def test_sys_rpo_coin_rs_matches_the_header_and_the_generator():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_rust_sys
    text = open(gen_rust_sys.RPO_COIN_OUT).read()
    assert text == gen_rust_sys.render_rpo_coin(gen_rust_sys.rpo_coin_prototypes())
    block = text[text.index('extern "C" {'):]
    rust = {m.group(1): [tuple(x.strip() for x in a.split(":", 1)) for a in m.group(2).split(",")]
            for m in re.finditer(r"pub fn (ms_[a-z0-9_]+)\((.*?)\)\s*->\s*c_int;", block)}
    c = _prototypes()
    assert sorted(rust) == sorted(c)
    for name, params in c.items():
        assert len(rust[name]) == len(params), name
        for cp, (rname, rtype) in zip(params, rust[name]):
            m = re.match(r"(.*?)([A-Za-z_][A-Za-z0-9_]*)$", cp)
            assert rname.rstrip("_") == m.group(2) and rtype == _expect(m.group(1).strip()), (name, cp, rname, rtype)
    assert "pub struct ms_rpo_coin_state { pub s: [u64; 12], pub pos: u32, pub pad: [u32; 7] }" in text
    assert "pub mod sys_rpo_coin;" in open(os.path.join(ROOT, "rust", "gpu", "src", "hip", "mod.rs")).read()
    # the five older files still come out of the generator as committed
    assert open(gen_rust_sys.OUT).read() == gen_rust_sys.render(gen_rust_sys.prototypes(open(gen_rust_sys.HEADER).read()))
    assert open(gen_rust_sys.TRANSCRIPT_OUT).read() == gen_rust_sys.render_transcript(gen_rust_sys.transcript_prototypes())
    assert open(gen_rust_sys.KECCAK_OUT).read() == gen_rust_sys.render_keccak(gen_rust_sys.keccak_prototypes())
    assert open(gen_rust_sys.EXT_OUT).read() == gen_rust_sys.render_ext(gen_rust_sys.ext_prototypes())
    assert open(gen_rust_sys.LOGUP_OUT).read() == gen_rust_sys.render_logup(gen_rust_sys.logup_prototypes())
