"""Starknet's Poseidon (the Hades permutation, t = 3, x^3, 8 full and 83 partial rounds) over p = 2^251 + 17 * 2^192 + 1, in Python
integers from the recipe alone: the reference of tests/test_poseidon252.py and the prover tests.  It never calls the library.

    rc[i] = int(sha256(b"Hades%d" % i).hexdigest(), 16) mod p,  i = 0 .. 272
    round r = 0 .. 90:  s[j] += rc[3r + j];  x -> x^3 on all of s when r < 4 or r >= 87, on s[2] alone otherwise;
                        mix with M = [[3, 1, 1], [1, -1, 1], [1, 1, -2]]
    hash2(x, y) = permute(x, y, 2)[0]
    hash_many(v): append 1, then 0 if the length is odd; from (0, 0, 0), for each pair (a, b): s0 += a, s1 += b, permute; -> s0
"""
import hashlib

P = (1 << 251) + 17 * (1 << 192) + 1
R = 1 << 256
ROUNDS = 91
RC = [int(hashlib.sha256(b"Hades%d" % i).hexdigest(), 16) % P for i in range(3 * ROUNDS)]


def permute(s0, s1, s2):
    for r in range(ROUNDS):
        s0, s1, s2 = (s0 + RC[3 * r]) % P, (s1 + RC[3 * r + 1]) % P, (s2 + RC[3 * r + 2]) % P
        if r < 4 or r >= 87:
            s0, s1 = pow(s0, 3, P), pow(s1, 3, P)
        s2 = pow(s2, 3, P)
        t = s0 + s1 + s2
        s0, s1, s2 = (t + 2 * s0) % P, (t - 2 * s1) % P, (t - 3 * s2) % P
    return s0, s1, s2


def hash2(x, y):
    return permute(x, y, 2)[0]


def hash_many(v):
    v = list(v) + [1]
    if len(v) % 2:
        v.append(0)
    s = (0, 0, 0)
    for k in range(0, len(v), 2):
        s = permute((s[0] + v[k]) % P, (s[1] + v[k + 1]) % P, s[2])
    return s[0]


# ---- the library's element form: four little-endian u64 words, Montgomery radix 2^256 ------------------------------------------------

def to_words(x):
    """canonical integer -> the four Montgomery words"""
    m = (x * R) % P
    return [(m >> (64 * k)) & ((1 << 64) - 1) for k in range(4)]


def from_words(w):
    """four Montgomery words -> canonical integer"""
    m = sum(int(x) << (64 * k) for k, x in enumerate(w))
    return (m * pow(R, -1, P)) % P


def digest_bytes(x):
    """the 32 bytes of a digest (a leaf or a node) as they lie in device memory"""
    return b"".join(w.to_bytes(8, "little") for w in to_words(x))


def digest_value(b):
    return from_words([int.from_bytes(b[8 * k: 8 * k + 8], "little") for k in range(4)])


def merkle_nodes(leaves):
    """nodes[k] = hash2(nodes[2k], nodes[2k+1]) over the leaf integers; nodes[0] = 0, nodes[1] the root"""
    n = len(leaves)
    nodes = [0] * n
    level = list(leaves)
    while len(level) > 1:
        level = [hash2(level[2 * i], level[2 * i + 1]) for i in range(len(level) // 2)]
        nodes[len(level): 2 * len(level)] = level
    return nodes
