"""BLAKE3 (unkeyed, default hash mode, 32-byte output) restated for the tests, independent of the library: a scalar form in plain
Python integers and a numpy form that runs N independent compressions at once on uint32 arrays (a 2^18-leaf tree in scalar Python
would take minutes).  tests/test_blake3.py pins the scalar form to tests/golden/blake3_kat.json and the batched form to the scalar one.

    compress(cv, m[16], counter, block_len, flags):  v = cv[0..8] || IV[0..4] || counter_lo, counter_hi, block_len, flags;
        7 rounds of four column G and four diagonal G (BLAKE2s's G), m permuted between rounds by m'[i] = m[P[i]];  cv' = v[i] ^ v[i + 8]
    chunks of 1024 bytes (empty input: one empty chunk), 64-byte blocks, the last zero-padded with block_len = its real bytes; every
        block of chunk c has counter c; CHUNK_START on a chunk's first block, CHUNK_END on its last
    parents compress(IV, left || right, 0, 64, PARENT); the left subtree takes the largest power of two of chunks below the count
    ROOT on the last compression only
Coin is the public coin's rules (tests/coin_ref.py) with this hash."""
import struct

import numpy as np

from tests import coin_ref

IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
PERM = (2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)
CHUNK_START, CHUNK_END, PARENT, ROOT = 1, 2, 4, 8
M32 = 0xFFFFFFFF
# the eight G of a round: (a, b, c, d) and the two message words each takes
ROUND = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def compress(cv, m, counter, block_len, flags):
    """cv: 8 words, m: 16 words -> the new 8-word chaining value"""
    v = list(cv) + list(IV[:4]) + [counter & M32, (counter >> 32) & M32, block_len, flags]
    m = list(m)
    for r in range(7):
        for g, (a, b, c, d) in enumerate(ROUND):
            v[a] = (v[a] + v[b] + m[2 * g]) & M32
            v[d] = _rotr(v[d] ^ v[a], 16)
            v[c] = (v[c] + v[d]) & M32
            v[b] = _rotr(v[b] ^ v[c], 12)
            v[a] = (v[a] + v[b] + m[2 * g + 1]) & M32
            v[d] = _rotr(v[d] ^ v[a], 8)
            v[c] = (v[c] + v[d]) & M32
            v[b] = _rotr(v[b] ^ v[c], 7)
        m = [m[PERM[i]] for i in range(16)]
    return [v[i] ^ v[i + 8] for i in range(8)]


def _chunk_cv(chunk, counter, root):
    """the chaining value of one chunk of 0..1024 bytes; root: it is the only chunk"""
    nblocks = max(1, (len(chunk) + 63) // 64)
    cv = list(IV)
    for b in range(nblocks):
        block = chunk[64 * b: 64 * b + 64]
        flags = (CHUNK_START if b == 0 else 0) | (CHUNK_END if b == nblocks - 1 else 0) | (ROOT if root and b == nblocks - 1 else 0)
        cv = compress(cv, struct.unpack("<16I", block.ljust(64, b"\0")), counter, len(block), flags)
    return cv


def _subtree(data, first_chunk, root):
    nchunks = max(1, (len(data) + 1023) // 1024)
    if nchunks == 1:
        return _chunk_cv(data, first_chunk, root)
    left = 1
    while 2 * left < nchunks:
        left *= 2
    a = _subtree(data[: 1024 * left], first_chunk, False)
    b = _subtree(data[1024 * left:], first_chunk + left, False)
    return compress(IV, a + b, 0, 64, PARENT | (ROOT if root else 0))


def blake3(data):
    """the 32-byte digest of `data`, scalar"""
    return struct.pack("<8I", *_subtree(bytes(data), 0, True))


# ---- N independent compressions at once --------------------------------------------------------------------------------------------

def _rotr_np(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def compress_many(cv, m, counter, block_len, flags):
    """cv: (N, 8) uint32, m: (N, 16) uint32; counter, block_len, flags: integers or (N,) arrays -> (N, 8) uint32"""
    n = m.shape[0]
    v = np.empty((16, n), dtype=np.uint32)
    v[:8] = np.asarray(cv, dtype=np.uint32).T
    for i in range(4):
        v[8 + i] = IV[i]
    v[12] = np.asarray(counter, dtype=np.uint64) & np.uint64(M32)
    v[13] = np.asarray(counter, dtype=np.uint64) >> np.uint64(32)
    v[14] = block_len
    v[15] = flags
    w = [np.ascontiguousarray(m[:, i], dtype=np.uint32) for i in range(16)]
    for r in range(7):
        for g, (a, b, c, d) in enumerate(ROUND):
            v[a] = v[a] + v[b] + w[2 * g]
            v[d] = _rotr_np(v[d] ^ v[a], 16)
            v[c] = v[c] + v[d]
            v[b] = _rotr_np(v[b] ^ v[c], 12)
            v[a] = v[a] + v[b] + w[2 * g + 1]
            v[d] = _rotr_np(v[d] ^ v[a], 8)
            v[c] = v[c] + v[d]
            v[b] = _rotr_np(v[b] ^ v[c], 7)
        w = [w[PERM[i]] for i in range(16)]
    return np.ascontiguousarray((v[:8] ^ v[8:]).T)


def _iv_rows(n):
    return np.tile(np.array(IV, dtype=np.uint32), (n, 1))


def blake3_many(msgs):
    """msgs: (N, L) uint8, N messages of the same length L -> (N, 32) uint8 digests.  Every message walks the same chunks, blocks and
    parents, so each step is one compress_many."""
    msgs = np.ascontiguousarray(msgs, dtype=np.uint8)
    n, L = msgs.shape
    nchunks = max(1, (L + 1023) // 1024)

    def chunk_cv(c, root):
        lo, hi = 1024 * c, min(L, 1024 * c + 1024)
        nblocks = max(1, (hi - lo + 63) // 64)
        cv = _iv_rows(n)
        for b in range(nblocks):
            b0, b1 = lo + 64 * b, min(hi, lo + 64 * b + 64)
            block = np.zeros((n, 64), dtype=np.uint8)
            block[:, : b1 - b0] = msgs[:, b0:b1]
            flags = (CHUNK_START if b == 0 else 0) | (CHUNK_END if b == nblocks - 1 else 0) | (ROOT if root and b == nblocks - 1 else 0)
            cv = compress_many(cv, block.view("<u4"), c, b1 - b0, flags)
        return cv

    def subtree(c0, count, root):
        if count == 1:
            return chunk_cv(c0, root)
        left = 1
        while 2 * left < count:
            left *= 2
        a, b = subtree(c0, left, False), subtree(c0 + left, count - left, False)
        return compress_many(_iv_rows(n), np.concatenate([a, b], axis=1), 0, 64, PARENT | (ROOT if root else 0))

    return np.ascontiguousarray(subtree(0, nchunks, True).astype("<u4")).view(np.uint8).reshape(n, 32)


def merkle_nodes(leaves):
    """leaves: (n, 32) uint8, n = 2^k >= 2 -> (n, 32) uint8 with nodes[k] = H(nodes[2k] || nodes[2k+1]), nodes[0] zero: a level at a time"""
    leaves = np.ascontiguousarray(leaves, dtype=np.uint8)
    n = leaves.shape[0]
    nodes = np.zeros((n, 32), dtype=np.uint8)
    cur = leaves
    count = n // 2
    while count >= 1:
        cur = blake3_many(cur.reshape(count, 64))                # a merge is the plain hash of 64 bytes: one compression
        nodes[count: 2 * count] = cur
        count //= 2
    return nodes


def leading_zero_bits(d):
    z = 0
    for b in d:
        if b:
            return z + 8 - b.bit_length()
        z += 8
    return z


def pow_search(seed, bits, batch=4096):
    """the smallest nonce >= 1 with `bits` leading zero bits of H(seed || nonce as 8 big-endian bytes)"""
    seed = np.frombuffer(bytes(seed), dtype=np.uint8)
    base = 1
    while True:
        nonces = np.arange(base, base + batch, dtype=np.uint64)
        msgs = np.empty((batch, 40), dtype=np.uint8)
        msgs[:, :32] = seed
        msgs[:, 32:] = nonces.astype(">u8").view(np.uint8).reshape(batch, 8)
        d = blake3_many(msgs)
        for i in range(batch):
            if leading_zero_bits(d[i].tobytes()) >= bits:
                return base + i
        base += batch


# ---- the public coin with H = BLAKE3 ------------------------------------------------------------------------------------------------


class Coin(coin_ref.Coin):
    """tests/coin_ref.Coin with H = BLAKE3.  coin_ref.py reaches its hash through a module-level function that knows two names, so
    every rule that hashes -- the word stream, the three reseeds, the proof-of-work search -- is restated here over blake3(); the
    samplers (draw, draw_queries), which only consume words, are the base class's."""

    def __init__(self, seed):
        super().__init__(seed, "blake3_256")

    def word(self):
        if not self.unread:
            self.counter += 1
            self.unread = blake3(self.seed + self.counter.to_bytes(8, "big"))
        popped = self.unread[-8:][::-1]                      # pop() takes the last byte first
        self.unread = self.unread[:-8]
        return int.from_bytes(popped, "big")

    def reseed_digest(self, d):
        assert len(d) == 32
        self._reset(blake3(self.seed + bytes(d)))

    def reseed_int(self, v):
        self._reset(blake3(self.seed + int(v).to_bytes(8, "big")))

    def reseed_elements(self, field, mont_words):
        V = {coin_ref.FP: 1, coin_ref.FQ3: 3, coin_ref.FP252: 4}[field]
        w = [int(x) for x in mont_words]
        assert len(w) % V == 0
        for i in range(0, len(w), V):
            self._reset(blake3(self.seed + blake3(coin_ref.element_bytes(field, w[i:i + V]))))

    def grind(self, bits):
        return pow_search(self.seed, bits)
