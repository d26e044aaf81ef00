"""The host logic that the byte hashes share (ministark_amd/csrc/commit_host.h): ONE Merkle level / subtree schedule and ONE windowed
proof-of-work search behind ms_sha256_*, ms_blake2s_*, ms_keccak_* and ms_coin_pow_grind.

1. The schedule.  A tree over 2^k random leaves is built under the profiler; the numbers of *_merkle_level and *_merkle_top launches
   are compared with a table derived by hand from the rules (NT = 256 parents per workgroup):
     count = 2^(k-1) parents.  count > 2^17: one level launch per level down to 2^17.  Then subtrees of NT parents, PER = 2 (two parents
     per lane) when the tree has <= 2^21 leaves, more than 256 subtrees and count % 512 == 0; they end in count / (PER NT) nodes, whose
     count / (2 PER NT) parents are <= NT and close the tree in one more launch.  count <= NT: that closing launch alone.
       k =  9: 256 parents                                              -> 0 level, 1 top
       k = 10: 512 parents = 2 subtrees (PER 1) -> 2 nodes -> 1 parent  -> 0 level, 2 top
       k = 18: 2^17 parents = 512 subtrees > 256: PER 2 -> 256 nodes    -> 0 level, 2 top
       k = 19: 2^18 parents: one level launch, then as k = 18           -> 1 level, 2 top
       k = 22: 2^21 .. 2^18 parents: four level launches; 2^22 > 2^21 leaves: PER 1 on 512 workgroups -> 512 nodes -> 256 parents
                                                                        -> 4 level, 2 top
   and every node is compared with the host reference of the hash's own tests: oracle.cref.sha256_merkle, hashlib.blake2s,
   hashlib.sha3_256, tests/keccak_ref.py.  From 2^18 leaves on the reference's nodes are a fixture, tests/golden/commit_schedule_nodes.json
   (one SHA-256 per level of the reference's node array: the host's Keccak-256 needs over a minute for 2^22 leaves); the leaves come from
   a seeded generator and `python -m tests.test_commit_schedule` records the file again from the same references.
2. ms_sha256_rows refuses a null column pointer before anything is enqueued, as its twins always did.
3. The search's windows: 2^12 nonces, then 2^14, ...; the second window starts at nonce 4097.  bits = 9; expected nonces come from a linear
   search with hashlib / keccak_ref.  Two seeds per hash, found once on the host and checked here by that search before they are used:
   NEAR's smallest nonce lies well inside the first window, FAR's in the second."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import cref
from tests import backends, keccak_ref
from ministark_amd import GOLDILOCKS_FP as FP, DeviceBytes, GpuVec, MerkleTree, grind_proof_of_work
from ministark_amd._lib import MsError
from ministark_amd.coin import PublicCoin

HASHES = ["sha256", "blake2s", "keccak256", "sha3_256"]
PREFIX = {"sha256": "sha256", "blake2s": "blake2s", "keccak256": "keccak", "sha3_256": "keccak"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "commit_schedule_nodes.json")
GOLDEN_FROM = 18                       # log2 leaves from which the expected nodes are the recorded fixture

# k -> (level launches, top launches); see the derivation above
SCHEDULE = {9: (0, 1), 10: (0, 2), 18: (0, 2), 19: (1, 2), 22: (4, 2)}


def hmany(hash, msgs):
    if hash == "keccak256":
        return keccak_ref.sponge256_many(msgs, 0x01)
    f = {"sha256": hashlib.sha256, "blake2s": hashlib.blake2s, "sha3_256": hashlib.sha3_256}[hash]
    return [f(m).digest() for m in msgs]


def _leaves(k):
    return np.random.default_rng(1000 + k).integers(0, 256, size=(1 << k) * 32, dtype=np.uint8)


def _reference_levels(hash, raw):
    """the reference's tree over the leaf bytes `raw`: -> [(count, bytes of nodes[count .. 2 count))] from the widest level to the root"""
    n = raw.size // 32
    if hash == "sha256":
        nodes = cref.sha256_merkle(raw.reshape(n, 32))
        return [(c, nodes[c: 2 * c].tobytes()) for c in (n >> s for s in range(1, n.bit_length()))]
    out = []
    level = [raw[32 * i: 32 * i + 32].tobytes() for i in range(n)]
    while len(level) > 1:
        level = hmany(hash, [level[2 * i] + level[2 * i + 1] for i in range(len(level) // 2)])
        out.append((len(level), b"".join(level)))
    return out


_golden = None


def _expected_levels(hash, k, raw):
    """-> [(count, expected, digest_only)]: the level's bytes, or for the recorded sizes the SHA-256 of them"""
    global _golden
    if k < GOLDEN_FROM:
        return [(c, b, False) for c, b in _reference_levels(hash, raw)]
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)
    digests = _golden[hash][str(k)]
    assert len(digests) == k
    return [((1 << k) >> (s + 1), bytes.fromhex(d), True) for s, d in enumerate(digests)]


def _schedule_case(kind, hash, k):
    pl = backends.planner(kind)
    n = 1 << k
    raw = _leaves(k)
    lv = DeviceBytes(pl, n * 32)
    pl.lib.check(pl.lib.ms_upload(pl.handle, lv.ptr, raw.ctypes.data, n * 32))
    pl.profile(True)
    try:
        tree = MerkleTree(pl, lv, n, hash)
        prof = pl.profile_read()
    finally:
        pl.profile(False)
    calls = {name: rec["calls"] for name, rec in prof.items()}
    got_launches = (calls.pop(PREFIX[hash] + "_merkle_level", 0), calls.pop(PREFIX[hash] + "_merkle_top", 0))
    print(f"{kind} {hash} 2^{k}: level launches {got_launches[0]}, top launches {got_launches[1]}, others {calls}")
    assert got_launches == SCHEDULE[k]
    assert not calls, "a tree is level and top launches only"
    got = tree.nodes_numpy()
    assert not got[0].any(), "nodes[0] must stay zero"
    for count, want, digest_only in _expected_levels(hash, k, raw):
        level = got[count: 2 * count].tobytes()
        assert (hashlib.sha256(level).digest() if digest_only else level) == want, f"level of {count} nodes"


@pytest.mark.parametrize("k", [9, 10, 18, 19])
@pytest.mark.parametrize("hash", HASHES)
def test_one_schedule_emu(hash, k):
    _schedule_case("emu", hash, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [9, 10, 18, 19, 22])
@pytest.mark.parametrize("hash", HASHES)
def test_one_schedule_hip(hash, k):
    _schedule_case("hip", hash, k)


def test_the_fixture_is_the_reference_at_its_smallest_size():
    """the recorded digests are what the references give today, for every hash (2^18 leaves: a second with hashlib and the C oracle, a
    few with keccak_ref's numpy lanes)"""
    raw = _leaves(GOLDEN_FROM)
    for hash in HASHES:
        want = [hashlib.sha256(b).digest() for _, b in _reference_levels(hash, raw)]
        assert [w for _, w, _ in _expected_levels(hash, GOLDEN_FROM, raw)] == want, hash


# ---- 2. the drift that the shared rows() closes ---------------------------------------------------------------------------------------

def test_sha256_rows_refuses_a_null_column_emu():
    pl = backends.planner("emu")
    L = pl.lib
    col = GpuVec.from_numpy(pl, cref.random_elements(8, 1))
    out = DeviceBytes(pl, 8 * 32)
    mark = bytes(range(1, 33)) * 8
    L.check(L.ms_upload(pl.handle, out.ptr, mark, len(mark)))
    cols = (ctypes.c_void_p * 3)(col.ptr, None, col.ptr)
    assert L.ms_sha256_rows(pl.handle, FP, 8, cols, 3, out.ptr) == -1                   # MS_ERR_INVALID
    with pytest.raises(MsError, match="ms_sha256_rows: null column 1") as e:
        L.check(L.ms_sha256_rows(pl.handle, FP, 8, cols, 3, out.ptr))
    assert e.value.code == -1
    assert out.to_numpy().tobytes() == mark, "nothing may be enqueued"
    assert L.ms_sha256_rows(pl.handle, FP, 8, (ctypes.c_void_p * 1)(None), 1, out.ptr) == -1      # the shape of the BLAKE2s assertion
    assert out.to_numpy().tobytes() == mark


# ---- 3. the windows of the search ---------------------------------------------------------------------------------------------------

BITS = 9
WINDOW0 = 1 << 12                      # nonces 1 .. 4096; the second window is 4097 .. 4097 + 2^14 - 1
# found once with the search below over seeds SHA-256("commit-schedule" || hash || i); the test checks where their smallest nonces lie
SEED_INDEX = {"sha256": (0, 2464), "blake2s": (0, 1127), "keccak256": (0, 2606), "sha3_256": (0, 5190)}


def _seed(hash, i):
    return hashlib.sha256(b"commit-schedule" + hash.encode() + i.to_bytes(4, "big")).digest()


def _lz(d):
    return 256 - int.from_bytes(d, "big").bit_length()


def _first_nonce(hash, seed, bits, limit):
    """the smallest nonce in [1, limit] with `bits` leading zero bits of H(seed || nonce as 8 big-endian bytes), or None"""
    for lo in range(1, limit + 1, 4096):
        block = range(lo, min(lo + 4096, limit + 1))
        for nonce, d in zip(block, hmany(hash, [seed + v.to_bytes(8, "big") for v in block])):
            if _lz(d) >= bits:
                return nonce
    return None


_answers = {}


def _seeds(hash):
    """-> (NEAR, its nonce, FAR, its nonce), searched once per hash"""
    if hash not in _answers:
        near, far = (_seed(hash, i) for i in SEED_INDEX[hash])
        n_near = _first_nonce(hash, near, BITS, WINDOW0 + (1 << 14))
        n_far = _first_nonce(hash, far, BITS, WINDOW0 + (1 << 14))
        assert n_near is not None and n_near < WINDOW0 - 1, "NEAR must hit inside the first window"
        assert n_far is not None and n_far > WINDOW0 + 1, "FAR must hit in the second window, past the boundary cases"
        _answers[hash] = (near, n_near, far, n_far)
    return _answers[hash]


def _grinders(pl, hash):
    """the two routes to the search: the seed in PowParams, the seed in a coin's state"""
    def direct(seed, max_nonce):
        return grind_proof_of_work(pl, seed, BITS, max_nonce, hash=hash)

    def coin(seed, max_nonce):
        c = PublicCoin(pl, seed, hash)
        try:
            return c.grind(BITS, max_nonce)
        finally:
            c.close()
    return {PREFIX[hash] + "_pow_grind": direct, "coin_pow_grind": coin}


def _grind_launches(pl, label, grind, seed, max_nonce):
    """-> (the nonce or None when the search refuses, the number of launches it took)"""
    pl.profile(True)
    try:
        try:
            nonce = grind(seed, max_nonce)
        except MsError as e:
            assert e.code == -1 and "no nonce below" in str(e), e
            nonce = None
        calls = pl.profile_read().get(label, {}).get("calls", 0)
    finally:
        pl.profile(False)
    return nonce, calls


def _windows_case(kind, hash):
    pl = backends.planner(kind)
    near, n_near, far, n_far = _seeds(hash)
    for label, grind in _grinders(pl, hash).items():
        # max_nonce below, on and above the first window's end: NEAR is found in one launch whatever the bound ...
        for max_nonce in (WINDOW0 - 1, WINDOW0, WINDOW0 + 1):
            got = _grind_launches(pl, label, grind, near, max_nonce)
            print(f"{kind} {label} {hash} near max_nonce {max_nonce}: {got}")
            assert got == (n_near, 1), (label, max_nonce)
        # ... and FAR is not there: one launch up to 4096, a second one (of a single nonce) for 4097
        for max_nonce, launches in ((WINDOW0 - 1, 1), (WINDOW0, 1), (WINDOW0 + 1, 2)):
            got = _grind_launches(pl, label, grind, far, max_nonce)
            print(f"{kind} {label} {hash} far max_nonce {max_nonce}: {got}")
            assert got == (None, launches), (label, max_nonce)
        # the smallest nonce in the second window; a bound one short of it holds no hit
        assert _grind_launches(pl, label, grind, far, 1 << 40) == (n_far, 2), label
        assert _grind_launches(pl, label, grind, far, n_far) == (n_far, 2), label
        assert _grind_launches(pl, label, grind, far, n_far - 1) == (None, 2), label
        with pytest.raises(MsError, match="no nonce below") as e:
            grind(far, n_far - 1)
        assert e.value.code == -1                                                        # MS_ERR_INVALID


@pytest.mark.parametrize("hash", HASHES)
def test_grinder_windows_emu(hash):
    _windows_case("emu", hash)


@pytest.mark.gpu
@pytest.mark.parametrize("hash", HASHES)
def test_grinder_windows_hip(hash):
    _windows_case("hip", hash)


# ---- recording the fixture --------------------------------------------------------------------------------------------------------------

def record_golden():
    out = {}
    for hash in HASHES:
        out[hash] = {}
        for k in sorted(k for k in SCHEDULE if k >= GOLDEN_FROM):
            out[hash][str(k)] = [hashlib.sha256(b).hexdigest() for _, b in _reference_levels(hash, _leaves(k))]
            print(hash, k, out[hash][str(k)][-1], flush=True)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    record_golden()
