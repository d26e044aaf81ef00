"""`PublicCoinImpl<F, H>` (src/random.rs:61-141) as `ProverChannel` uses it (src/channel.rs:46-100, src/fri.rs:217-247), with its state
in device memory: the ms_coin_* entry points of include/ministark_hip_transcript.h.  A commitment's root is absorbed where the tree builder left it
(`MerkleTree.root_ptr()`), a drawn challenge stays on the device (`draw` returns a GpuVec that `api.apply_drp` hands to
ms_fri_fold_dev), and none of the reseeds or draws waits for the device."""
import ctypes

import numpy as np

from . import _lib
from .api import FIELD_WORDS, DeviceBytes, GpuVec

HASH_IDS = {"sha256": 0, "blake2s": 1, "keccak256": 3, "sha3_256": 4}        # 2 is left for an RPO-256 coin


class PublicCoin:
    """`PublicCoin::new(seed)` (src/random.rs:102-109).  seed32: 32 bytes; hash: "sha256" (Sha256HashFn), "blake2s", "keccak256" or "sha3_256"."""

    def __init__(self, planner, seed32, hash="sha256"):
        if hash not in HASH_IDS:
            raise ValueError(f"unknown coin hash {hash!r} (one of {sorted(HASH_IDS)})")
        seed32 = bytes(seed32)
        if len(seed32) != 32:
            raise ValueError("the coin's seed is a 32-byte digest")
        self.planner, self.hash = planner, hash
        h = ctypes.c_void_p()
        planner.lib.check(planner.lib.ms_coin_create(planner.handle, HASH_IDS[hash], ctypes.create_string_buffer(seed32, 32), ctypes.byref(h)))
        self.ptr = h.value

    def _call(self, fn, *args):
        self.planner.lib.check(fn(self.planner.handle, self.ptr, *args))

    def reseed_digest(self, digest):
        """`reseed_with_digest`: digest is a DeviceBytes (its first 32 bytes) or a device address, e.g. `tree.root_ptr()`.  Asynchronous."""
        self._call(self.planner.lib.ms_coin_reseed_digest, digest.ptr if isinstance(digest, DeviceBytes) else int(digest))

    def reseed_int(self, value):
        """`reseed_with_int` (the proof-of-work nonce).  Asynchronous."""
        self._call(self.planner.lib.ms_coin_reseed_int, int(value))

    def reseed_elements(self, elems, field=None):
        """`reseed_with_field_elements`: a GpuVec, or numpy u64 Montgomery words of `field` elements on the host.  Asynchronous."""
        L = self.planner.lib
        if isinstance(elems, GpuVec):
            self._call(L.ms_coin_reseed_elements, elems.field, elems.ptr, len(elems))
            return
        if field is None:
            raise ValueError("reseed_elements: host elements need their field")
        arr = np.ascontiguousarray(elems, dtype=np.uint64).ravel()
        assert arr.size % FIELD_WORDS[field] == 0
        self._call(L.ms_coin_reseed_elements_host, field, arr.ctypes.data, arr.size // FIELD_WORDS[field])

    def draw(self, field, count=1):
        """`draw()` x count -> GpuVec of `count` elements of `field` (Montgomery form), left on the device.  Asynchronous."""
        out = GpuVec(self.planner, count, field)
        self._call(self.planner.lib.ms_coin_draw, field, count, out.ptr)
        return out

    def draw_queries(self, max_n, domain_size):
        """`draw_queries(max_n, domain_size)`: the distinct positions in ascending order.  Blocks."""
        pos = np.empty(max(max_n, 1), dtype=np.uint64)
        n = ctypes.c_size_t(0)
        self._call(self.planner.lib.ms_coin_draw_queries, max_n, domain_size, pos.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(n))
        return [int(p) for p in pos[: n.value]]

    def grind(self, bits, max_nonce=1 << 40):
        """`grind_proof_of_work(bits)`: the smallest nonce >= 1; the coin is not reseeded (channel.rs:86-93 does that).  Blocks."""
        out = ctypes.c_uint64(0)
        self._call(self.planner.lib.ms_coin_pow_grind, bits, max_nonce, ctypes.byref(out))
        return out.value

    def state(self):
        """-> dict(seed=bytes, counter=int, unread=bytes): the unread bytes are consumed from the end.  Blocks."""
        st = _lib.CoinState()
        self._call(self.planner.lib.ms_coin_read, ctypes.byref(st))
        return {"seed": bytes(st.seed), "counter": int(st.counter), "unread": bytes(st.bytes)[: st.nbytes]}

    def set_state(self, seed, counter, unread=b""):
        """ms_coin_write: replace the state (tests, checkpoints); len(unread) in {0, 8, 16, 24, 32}."""
        st = _lib.CoinState()
        ctypes.memmove(st.seed, bytes(seed), 32)
        st.counter, st.nbytes = counter, len(unread)
        ctypes.memmove(st.bytes, bytes(unread).ljust(32, b"\0"), 32)
        self._call(self.planner.lib.ms_coin_write, ctypes.byref(st))

    def close(self):
        if self.ptr and self.planner.handle:
            self.planner.lib.ms_coin_destroy(self.planner.handle, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
