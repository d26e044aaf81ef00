"""The public coin's rules in plain Python (hashlib, big integers): the reference the device coin is compared with.  Written from
the rules as include/ministark_hip_transcript.h states them, not from the kernels.

  words          nothing unread: counter += 1, unread = H(seed || counter as 8 big-endian bytes); a word is 8 bytes popped from the END,
                 the first popped byte the most significant
  reseed_digest  seed = H(seed || d), counter = 0, nothing unread
  reseed_int     seed = H(seed || v as 8 big-endian bytes), counter = 0, nothing unread
  reseed_elements  per element: seed = H(seed || H(canonical little-endian bytes)), counter = 0, nothing unread
  draw           N words as limbs 0..N-1, top bits of the last limb cleared, accepted when < p; the limbs are the Montgomery residue
  draw_queries   max_n x { zone = (range << clz64(range)) - 1; words v until lo64(v range) <= zone; hi64(v range) }, distinct, ascending
Every draw reports how many samples it rejected (`rejections` of the last call, `first_try` how many were accepted at once)."""
import hashlib

GL_P = (1 << 64) - (1 << 32) + 1
F252_P = (1 << 251) + 17 * (1 << 192) + 1
GL_R, F252_R = 1 << 64, 1 << 256
M64 = (1 << 64) - 1
FP, FQ3, FP252 = 0, 1, 2


def H(hash, data):
    return (hashlib.sha256 if hash == "sha256" else hashlib.blake2s)(data).digest()


def element_bytes(field, mont_words):
    """canonical little-endian bytes of ONE element given as its Montgomery u64 words (1, 3 or 4 of them)"""
    w = [int(x) for x in mont_words]
    if field == FP252:
        m = sum(x << (64 * i) for i, x in enumerate(w))
        return (m * pow(F252_R, -1, F252_P) % F252_P).to_bytes(32, "little")
    return b"".join((x * pow(GL_R, -1, GL_P) % GL_P).to_bytes(8, "little") for x in w)


class Coin:
    def __init__(self, seed, hash="sha256"):
        assert len(seed) == 32
        self.hash, self.seed, self.counter, self.unread = hash, bytes(seed), 0, b""
        self.rejections, self.first_try = 0, 0

    def state(self):
        return {"seed": self.seed, "counter": self.counter, "unread": self.unread}

    def word(self):
        if not self.unread:
            self.counter += 1
            self.unread = H(self.hash, self.seed + self.counter.to_bytes(8, "big"))
        popped = self.unread[-8:][::-1]                      # pop() takes the last byte first
        self.unread = self.unread[:-8]
        return int.from_bytes(popped, "big")

    def _reset(self, seed):
        self.seed, self.counter, self.unread = seed, 0, b""

    def reseed_digest(self, d):
        assert len(d) == 32
        self._reset(H(self.hash, self.seed + bytes(d)))

    def reseed_int(self, v):
        self._reset(H(self.hash, self.seed + int(v).to_bytes(8, "big")))

    def reseed_elements(self, field, mont_words):
        V = {FP: 1, FQ3: 3, FP252: 4}[field]
        w = [int(x) for x in mont_words]
        assert len(w) % V == 0
        for i in range(0, len(w), V):
            self._reset(H(self.hash, self.seed + H(self.hash, element_bytes(field, w[i:i + V]))))

    def _draw_base(self, nlimbs, p, clear):
        tries = 0
        while True:
            limbs = [self.word() for _ in range(nlimbs)]
            limbs[-1] &= M64 >> clear
            if sum(x << (64 * i) for i, x in enumerate(limbs)) < p:
                self.rejections += tries
                self.first_try += tries == 0
                return limbs
            tries += 1

    def draw(self, field, count=1):
        """-> the Montgomery u64 words of `count` elements, flat"""
        self.rejections, self.first_try = 0, 0
        out = []
        for _ in range(count):
            if field == FP252:
                out += self._draw_base(4, F252_P, 4)
            else:
                for _ in range(3 if field == FQ3 else 1):
                    out += self._draw_base(1, GL_P, 0)
        return out

    def draw_queries(self, max_n, domain_size):
        self.rejections = 0
        zone = ((domain_size << (64 - domain_size.bit_length())) - 1) & M64
        got = set()
        for _ in range(max_n):
            while True:
                prod = self.word() * domain_size
                if prod & M64 <= zone:
                    got.add(prod >> 64)
                    break
                self.rejections += 1
        return sorted(got)

    def grind(self, bits):
        nonce = 1
        while True:
            d = int.from_bytes(H(self.hash, self.seed + nonce.to_bytes(8, "big")), "big")
            if 256 - d.bit_length() >= bits:
                return nonce
            nonce += 1
