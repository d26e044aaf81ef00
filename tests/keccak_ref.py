"""The Keccak sponge in plain Python with the domain byte as a parameter, and the public coin on top of it: the reference the
ms_keccak_* entry points and the Keccak / SHA3 coins are compared with.  Written from the rules of include/ministark_hip_keccak.h and
FIPS 202, not from the kernels:

  rate 136 bytes, capacity 512 bits, lanes little-endian; the domain byte (0x01 Keccak-256, 0x06 SHA3-256) at offset L mod 136 of the
  last block, 0x80 ORed into that block's byte 135; L = 0 mod 136 gives one more block of padding alone; digest = state[0..32).

tests/test_keccak.py pins this sponge first: with 0x06 it must equal hashlib.sha3_256, with 0x01 it must give the published
Keccak-256 digests of "" and "abc".  The coin restates the rules of DESIGN.md section 4.13 by overriding the one place
tests/coin_ref.py hashes (its module-level H falls back to BLAKE2s for a name it does not know, so it is never given these names)."""
from tests import coin_ref

M64 = (1 << 64) - 1
RATE = 136
DOMAIN = {"keccak256": 0x01, "sha3_256": 0x06}
HASH_IDS = {"keccak256": 3, "sha3_256": 4}

RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
      0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
      0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
      0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]


def _rotl(v, n):
    n %= 64
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def keccak_f(a):
    """Keccak-f[1600] on 25 lanes a[x + 5 y]; rho's offsets come from the (t + 1)(t + 2) / 2 walk of FIPS 202, not from a table"""
    for rc in RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        b[0] = a[0]
        x, y = 1, 0
        for t in range(24):
            b[y + 5 * ((2 * x + 3 * y) % 5)] = _rotl(a[x + 5 * y], (t + 1) * (t + 2) // 2)
            x, y = y, (2 * x + 3 * y) % 5
        a = [b[i] ^ (~b[(i % 5 + 1) % 5 + 5 * (i // 5)] & M64 & b[(i % 5 + 2) % 5 + 5 * (i // 5)]) for i in range(25)]
        a[0] ^= rc
    return a


def sponge256(data, domain):
    """the 32-byte digest of `data` under the Keccak[512] sponge with the given domain byte"""
    data = bytes(data)
    pad = bytearray(RATE - len(data) % RATE)
    pad[0] = domain
    pad[-1] |= 0x80
    msg = data + bytes(pad)
    a = [0] * 25
    for off in range(0, len(msg), RATE):
        for i in range(RATE // 8):
            a[i] ^= int.from_bytes(msg[off + 8 * i: off + 8 * i + 8], "little")
        a = keccak_f(a)
    return b"".join(v.to_bytes(8, "little") for v in a[:4])


def sponge256_many(msgs, domain):
    """sponge256 of many messages of ONE length at once (numpy lanes, one array entry per message) -> list of 32-byte digests.  The same
    rules restated on arrays, so that a tree of 2^18 nodes or 257 rows of 4 KiB take milliseconds; pinned against hashlib and against
    sponge256 by the first test of tests/test_keccak.py."""
    import numpy as np
    msgs = [bytes(m) for m in msgs]
    if not msgs:
        return []
    L = len(msgs[0])
    assert all(len(m) == L for m in msgs)
    pad = bytearray(RATE - L % RATE)
    pad[0] = domain
    pad[-1] |= 0x80
    buf = np.frombuffer(b"".join(m + bytes(pad) for m in msgs), dtype="<u8").reshape(len(msgs), -1).astype(np.uint64)
    rot = lambda v, n: (v << np.uint64(n % 64)) | (v >> np.uint64(64 - n % 64)) if n % 64 else v
    a = [np.zeros(len(msgs), dtype=np.uint64) for _ in range(25)]
    for blk in range(buf.shape[1] // 17):
        for i in range(17):
            a[i] = a[i] ^ buf[:, 17 * blk + i]
        for rc in RC:
            c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
            d = [c[(x + 4) % 5] ^ rot(c[(x + 1) % 5], 1) for x in range(5)]
            a = [a[i] ^ d[i % 5] for i in range(25)]
            b = [None] * 25
            b[0] = a[0]
            x, y = 1, 0
            for t in range(24):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rot(a[x + 5 * y], (t + 1) * (t + 2) // 2)
                x, y = y, (2 * x + 3 * y) % 5
            a = [b[i] ^ (~b[(i % 5 + 1) % 5 + 5 * (i // 5)] & b[(i % 5 + 2) % 5 + 5 * (i // 5)]) for i in range(25)]
            a[0] = a[0] ^ np.uint64(rc)
    out = np.stack(a[:4], axis=1).astype("<u8")
    return [out[k].tobytes() for k in range(len(msgs))]


def H(hash, data):
    return sponge256(data, DOMAIN[hash])                      # KeyError for any other name: nothing falls back


def keccak256(data):
    return sponge256(data, 0x01)


def sha3_256(data):
    return sponge256(data, 0x06)


class Coin(coin_ref.Coin):
    """tests/coin_ref.Coin with H = Keccak-256 / SHA3-256: every rule (word stream, reseeds, samplers) is the base class's; only the
    hash differs.  The base class reaches its hash through the module-level coin_ref.H, which these methods never call."""

    def __init__(self, seed, hash):
        assert hash in DOMAIN
        super().__init__(seed, hash)

    def word(self):
        if not self.unread:
            self.counter += 1
            self.unread = H(self.hash, self.seed + self.counter.to_bytes(8, "big"))
        popped = self.unread[-8:][::-1]
        self.unread = self.unread[:-8]
        return int.from_bytes(popped, "big")

    def reseed_digest(self, d):
        assert len(d) == 32
        self._reset(H(self.hash, self.seed + bytes(d)))

    def reseed_int(self, v):
        self._reset(H(self.hash, self.seed + int(v).to_bytes(8, "big")))

    def reseed_elements(self, field, mont_words):
        V = {coin_ref.FP: 1, coin_ref.FQ3: 3, coin_ref.FP252: 4}[field]
        w = [int(x) for x in mont_words]
        assert len(w) % V == 0
        for i in range(0, len(w), V):
            self._reset(H(self.hash, self.seed + H(self.hash, coin_ref.element_bytes(field, w[i:i + V]))))

    def grind(self, bits):
        nonce = 1
        while True:
            d = int.from_bytes(H(self.hash, self.seed + nonce.to_bytes(8, "big")), "big")
            if 256 - d.bit_length() >= bits:
                return nonce
            nonce += 1
