"""TESTS ONLY: the RPO-256 public coin of include/ministark_hip_rpo_coin.h in Python integers on oracle.pyref.rpo.permute -- the rules
as the header states them, written without looking at the kernels.  Every value is a canonical Goldilocks integer.  The package never
imports this file."""
from oracle.pyref import rpo

P = rpo.P


class Coin:
    def __init__(self, seed4):
        seed4 = [int(v) for v in seed4]
        assert len(seed4) == 4 and all(0 <= v < P for v in seed4)
        self.s = rpo.permute([0, 0, 0, 0] + seed4 + [0, 0, 0, 0])
        self.pos = 4
        self.permutations = 1

    def copy(self):
        c = Coin.__new__(Coin)
        c.s, c.pos, c.permutations = list(self.s), self.pos, self.permutations
        return c

    def state(self):
        return {"s": list(self.s), "pos": self.pos}

    def _permute(self):
        self.s = rpo.permute(self.s)
        self.permutations += 1

    def _absorb(self, words):
        assert len(words) <= 8
        for j, w in enumerate(words):
            self.s[4 + j] = (self.s[4 + j] + w) % P
        self._permute()

    def reseed_digest(self, d4):
        assert len(d4) == 4
        self._absorb(list(d4))
        self.pos = 4

    def reseed_int(self, v):
        assert 0 <= v < 1 << 64
        self._absorb([v & 0xFFFFFFFF, v >> 32])
        self.pos = 4

    def reseed_elements(self, words):
        """words: the base-field words in memory order (c0, c1, c2 of each Fq3 element)."""
        words = [int(w) for w in words]
        if not words:
            return
        words = words + [1]
        words += [0] * (-len(words) % 8)
        for a in range(0, len(words), 8):
            self._absorb(words[a:a + 8])
        self.pos = 4

    def word(self):
        if self.pos == 12:
            self._permute()
            self.pos = 4
        w = self.s[self.pos]
        self.pos += 1
        return w

    def draw(self, nwords):
        return [self.word() for _ in range(nwords)]

    def draw_queries(self, max_n, domain_size):
        assert domain_size >= 1 and domain_size & (domain_size - 1) == 0 and domain_size <= 1 << 32
        return sorted({self.word() & (domain_size - 1) for _ in range(max_n)})

    def accepts(self, nonce, bits):
        t = list(self.s)
        t[4] = (t[4] + (nonce & 0xFFFFFFFF)) % P
        t[5] = (t[5] + (nonce >> 32)) % P
        return rpo.permute(t)[0] & ((1 << bits) - 1) == 0

    def grind(self, bits, max_nonce=1 << 40):
        """The linear search: the smallest accepted nonce in 1..max_nonce, or None."""
        for n in range(1, max_nonce + 1):
            if self.accepts(n, bits):
                return n
        return None
