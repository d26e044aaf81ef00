"""`PublicCoinImpl<F, H>` (src/random.rs:61-141) as `ProverChannel` uses it (src/channel.rs:46-100, src/fri.rs:217-247), with its state
in device memory: the ms_coin_* entry points of include/ministark_hip_transcript.h.  A commitment's root is absorbed where the tree builder left it
(`MerkleTree.root_ptr()`), a drawn challenge stays on the device (`draw` returns a GpuVec that `api.apply_drp` hands to
ms_fri_fold_dev), and none of the reseeds or draws waits for the device.  `RpoCoin` is the algebraic coin of
include/ministark_hip_rpo_coin.h (ms_rpo_coin_*): the same methods over an RPO-256 sponge that absorbs and draws field elements.
`PoseidonCoin` is the algebraic coin of the 252-bit field (include/ministark_hip_hades_coin.h, ms_hades_coin_*): the same methods over
one field element and a draw counter."""
import ctypes

import numpy as np

from . import _lib
from .api import F252_P, FIELD_WORDS, GL_P, DeviceBytes, GpuVec, f252_from_mont_limbs, f252_to_mont_limbs, gl_from_mont, gl_to_mont

HASH_IDS = {"sha256": 0, "blake2s": 1, "keccak256": 3, "sha3_256": 4, "blake3_256": 6}        # 2 and 5 stay unknown: the RPO-256 coin is RpoCoin, a family of its own


class _Coin:
    """What the three coins share: every method is the entry point `_prefix` + its name on the coin's handle, so `pipeline.prove` holds
    any of them.  A subclass creates the coin (`_create`) and knows its state struct (`state`, `set_state`)."""

    _prefix = None                                                              # "ms_coin_", "ms_rpo_coin_", "ms_hades_coin_"

    ptr = None                                                                  # until `_create` has returned, and after `close`

    def _create(self, planner, *args):
        self.planner = planner
        h = ctypes.c_void_p()
        planner.lib.check(getattr(planner.lib, self._prefix + "create")(planner.handle, *args, ctypes.byref(h)))
        self.ptr = h.value

    def _call(self, name, *args):
        self.planner.lib.check(getattr(self.planner.lib, self._prefix + name)(self.planner.handle, self.ptr, *args))

    def reseed_digest(self, digest):
        """`reseed_with_digest`: digest is a DeviceBytes (its first 32 bytes) or a device address, e.g. `tree.root_ptr()`.  Asynchronous."""
        self._call("reseed_digest", digest.ptr if isinstance(digest, DeviceBytes) else int(digest))

    def reseed_int(self, value):
        """`reseed_with_int` (the proof-of-work nonce).  Asynchronous."""
        self._call("reseed_int", int(value))

    def reseed_elements(self, elems, field=None):
        """`reseed_with_field_elements`: a GpuVec, or numpy u64 Montgomery words of `field` elements on the host.  Asynchronous."""
        if isinstance(elems, GpuVec):
            self._call("reseed_elements", elems.field, elems.ptr, len(elems))
            return
        if field is None:
            raise ValueError("reseed_elements: host elements need their field")
        arr = np.ascontiguousarray(elems, dtype=np.uint64).ravel()
        assert arr.size % FIELD_WORDS[field] == 0
        self._call("reseed_elements_host", field, arr.ctypes.data, arr.size // FIELD_WORDS[field])

    def draw(self, field, count=1):
        """`draw()` x count -> GpuVec of `count` elements of `field` (Montgomery form), left on the device.  Asynchronous."""
        out = GpuVec(self.planner, count, field)
        self._call("draw", field, count, out.ptr)
        return out

    def draw_queries(self, max_n, domain_size):
        """`draw_queries(max_n, domain_size)`: the distinct positions in ascending order.  Blocks."""
        pos = np.empty(max(max_n, 1), dtype=np.uint64)
        n = ctypes.c_size_t(0)
        self._call("draw_queries", max_n, domain_size, pos.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(n))
        return [int(p) for p in pos[: n.value]]

    def grind(self, bits, max_nonce=1 << 40):
        """`grind_proof_of_work(bits)`: the smallest nonce >= 1; the coin is not reseeded (channel.rs:86-93 does that).  Blocks."""
        out = ctypes.c_uint64(0)
        self._call("pow_grind", bits, max_nonce, ctypes.byref(out))
        return out.value

    def close(self):
        if self.ptr and self.planner.handle:
            getattr(self.planner.lib, self._prefix + "destroy")(self.planner.handle, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PublicCoin(_Coin):
    """`PublicCoin::new(seed)` (src/random.rs:102-109).  seed32: 32 bytes; hash: "sha256" (Sha256HashFn), "blake2s", "keccak256", "sha3_256" or "blake3_256"."""

    _prefix = "ms_coin_"

    def __init__(self, planner, seed32, hash="sha256"):
        if hash not in HASH_IDS:
            raise ValueError(f"unknown coin hash {hash!r} (one of {sorted(HASH_IDS)})")
        seed32 = bytes(seed32)
        if len(seed32) != 32:
            raise ValueError("the coin's seed is a 32-byte digest")
        self.hash = hash
        self._create(planner, HASH_IDS[hash], ctypes.create_string_buffer(seed32, 32))

    def state(self):
        """-> dict(seed=bytes, counter=int, unread=bytes): the unread bytes are consumed from the end.  Blocks."""
        st = _lib.CoinState()
        self._call("read", ctypes.byref(st))
        return {"seed": bytes(st.seed), "counter": int(st.counter), "unread": bytes(st.bytes)[: st.nbytes]}

    def set_state(self, seed, counter, unread=b""):
        """ms_coin_write: replace the state (tests, checkpoints); len(unread) in {0, 8, 16, 24, 32}."""
        st = _lib.CoinState()
        ctypes.memmove(st.seed, bytes(seed), 32)
        st.counter, st.nbytes = counter, len(unread)
        ctypes.memmove(st.bytes, bytes(unread).ljust(32, b"\0"), 32)
        self._call("write", ctypes.byref(st))


def rpo_seed(seed):
    """The seed of an `RpoCoin`: four canonical integers, or 32 bytes read as four little-endian u64; every word below p."""
    if isinstance(seed, (bytes, bytearray, memoryview)):
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError("the coin's seed is 32 bytes (four little-endian u64) or four integers")
        words = [int.from_bytes(seed[8 * k: 8 * k + 8], "little") for k in range(4)]
    else:
        words = [int(v) for v in seed]
        if len(words) != 4:
            raise ValueError("the coin's seed is 32 bytes (four little-endian u64) or four integers")
    if any(not 0 <= w < GL_P for w in words):
        raise ValueError("the words of an RPO-256 coin's seed are Goldilocks elements: below p")
    return words


class RpoCoin(_Coin):
    """The RPO-256 public coin (ms_rpo_coin_*): a 12-element sponge on the device, capacity s[0..4), rate s[4..12).  It has `PublicCoin`'s
    methods, so `pipeline.prove` holds either.  seed: see `rpo_seed`.  The rules are in include/ministark_hip_rpo_coin.h: `reseed_digest`
    absorbs four elements of device memory (the root of an RPO-256 tree), `reseed_int` a u64 as its two 32-bit halves, `reseed_elements`
    and `draw` work over Fp or Fq3, `draw_queries` takes a power of two up to 2^32, and `grind` finds the smallest nonce >= 1 after whose
    `reseed_int` s[0] has its low `bits` bits zero."""

    hash = "rpo256"
    _prefix = "ms_rpo_coin_"

    def __init__(self, planner, seed):
        self._create(planner, (ctypes.c_uint64 * 4)(*[gl_to_mont(w) for w in rpo_seed(seed)]))

    def state(self):
        """-> {"s": the 12 state elements as canonical integers, "pos": the next unread rate element (12: none)}.  Blocks."""
        st = _lib.RpoCoinState()
        self._call("read", ctypes.byref(st))
        return {"s": [gl_from_mont(int(w)) for w in st.s], "pos": int(st.pos)}

    def set_state(self, s, pos):
        """ms_rpo_coin_write: replace the state (tests, checkpoints); s: 12 canonical integers, pos in 4..12."""
        st = _lib.RpoCoinState()
        for k, v in enumerate(s):
            st.s[k] = gl_to_mont(int(v))
        st.pos = pos
        self._call("write", ctypes.byref(st))


def poseidon_seed(seed):
    """The seed of a `PoseidonCoin`: one element of the 252-bit field, as an integer below p or as 32 bytes read little-endian."""
    if isinstance(seed, (bytes, bytearray, memoryview)):
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError("the coin's seed is 32 bytes (one little-endian integer) or an integer")
        value = int.from_bytes(seed, "little")
    else:
        value = int(seed)
    if not 0 <= value < F252_P:
        raise ValueError("the seed of a Poseidon coin is an element of the 252-bit field: below p")
    return value


class PoseidonCoin(_Coin):
    """The Poseidon public coin of the 252-bit field (ms_hades_coin_*): one field element and a draw counter on the device.  It has
    `RpoCoin`'s methods, so `pipeline.prove` holds either.  seed: see `poseidon_seed`.  The rules are in
    include/ministark_hip_hades_coin.h: digest = hash2(digest, x) absorbs, permute(digest, n_draws + i, 3)[0] draws, tag 4 grinds.
    `reseed_digest` absorbs one element of device memory (the root of a "poseidon252" tree), `reseed_int` a u64, `reseed_elements` the
    hash_many of STARK252_FP elements; `draw` gives STARK252_FP elements, `draw_queries` takes a power of two up to 2^32, and `grind`
    finds the smallest nonce n >= 1 such that permute(digest, n, 4)[0] has its low `bits` bits zero."""

    hash = "poseidon252"
    _prefix = "ms_hades_coin_"

    def __init__(self, planner, seed):
        value = poseidon_seed(seed)
        self._create(planner, (ctypes.c_uint64 * 4)(*[(value >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]))      # canonical words: the library converts

    def state(self):
        """-> {"digest": the digest as a canonical integer, "n_draws": the draws made since the last reseed}.  Blocks."""
        st = _lib.HadesCoinState()
        self._call("read", ctypes.byref(st))
        return {"digest": f252_from_mont_limbs(st.digest), "n_draws": int(st.n_draws)}

    def set_state(self, digest, n_draws):
        """ms_hades_coin_write: replace the state (tests, checkpoints); digest: a canonical integer below p."""
        st = _lib.HadesCoinState()
        for k, v in enumerate(f252_to_mont_limbs(int(digest) % F252_P)):
            st.digest[k] = int(v)
        st.n_draws = n_draws
        self._call("write", ctypes.byref(st))
