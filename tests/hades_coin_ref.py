"""The Poseidon public coin of the 252-bit field (include/ministark_hip_hades_coin.h) restated in Python integers on
tests/poseidon_ref.py: the reference of tests/test_hades_coin.py and of the transcript replay of tests/test_hades_coin_prover.py.  It
never calls the library.

    state            one element `digest` and a counter `n_draws`
    create(seed)     digest = seed; n_draws = 0
    reseed_digest(d) digest = hash2(digest, d); n_draws = 0                       hash2(x, y) = permute(x, y, 2)[0]
    reseed_int(v)    digest = hash2(digest, v); n_draws = 0
    reseed_elements  digest = hash2(digest, hash_many(e)); n_draws = 0;  nothing at all for no element
    draw(count)      permute(digest, n_draws + i, 3)[0] for i < count; n_draws += count
    draw_queries     the distinct values of (draw & (domain_size - 1)) over max_n draws, ascending
    grind(bits)      the smallest n >= 1 with permute(digest, n, 4)[0] & (2^bits - 1) == 0
"""
from tests import poseidon_ref as pos

P = pos.P
TAG_ABSORB, TAG_DRAW, TAG_POW = 2, 3, 4


class Coin:
    def __init__(self, seed):
        assert 0 <= seed < P
        self.digest, self.n_draws, self.permutations = seed, 0, 0

    def copy(self):
        c = Coin(self.digest)
        c.n_draws, c.permutations = self.n_draws, self.permutations
        return c

    def state(self):
        return {"digest": self.digest, "n_draws": self.n_draws}

    def _absorb(self, y):
        self.digest = pos.permute(self.digest, y, TAG_ABSORB)[0]
        self.n_draws = 0
        self.permutations += 1

    def reseed_digest(self, d):
        assert 0 <= d < P
        self._absorb(d)

    def reseed_int(self, v):
        assert 0 <= v < 1 << 64
        self._absorb(v)

    def reseed_elements(self, elems):
        elems = list(elems)
        if not elems:
            return
        self.permutations += len(elems) // 2 + 1
        self._absorb(pos.hash_many(elems))

    def draw(self, count):
        assert self.n_draws + count - 1 < 1 << 64
        out = [pos.permute(self.digest, self.n_draws + i, TAG_DRAW)[0] for i in range(count)]
        self.n_draws = (self.n_draws + count) % (1 << 64)
        self.permutations += count
        return out

    def draw_queries(self, max_n, domain_size):
        assert domain_size & (domain_size - 1) == 0 and 1 <= domain_size <= 1 << 32
        return sorted({v & (domain_size - 1) for v in self.draw(max_n)})

    def accepts(self, nonce, bits):
        return pos.permute(self.digest, nonce, TAG_POW)[0] & ((1 << bits) - 1) == 0

    def grind(self, bits, max_nonce=1 << 40):
        """linear scan; None when no nonce in 1..max_nonce is accepted"""
        for n in range(1, max_nonce + 1):
            if self.accepts(n, bits):
                return n
        return None
