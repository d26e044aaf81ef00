"""BLAKE3 commitments and proof-of-work (ms_blake3_*, hash="blake3_256"): device against tests/blake3_ref.py, byte-exact.

H = unkeyed BLAKE3, default hash mode, 32-byte digest.  Leaf of row r = H(canonical little-endian bytes of every element of the row),
the bytes the SHA-256 / BLAKE2s leaves hash (Fp 8 bytes, Fq3 c0||c1||c2, Fp252 32 bytes) -- a row longer than 1024 bytes is BLAKE3's tree
of chunks, which is what the column counts below walk: every block edge and every chunk edge a row of at most 128 columns can reach;
nodes[k] = H(nodes[2k] || nodes[2k+1]), the plain hash of 64 bytes; the nonce is the smallest n >= 1 with `bits` leading zero bits of
H(seed || n as 8 big-endian bytes).  Expected values come from the helper, which the first test pins to tests/golden/blake3_kat.json,
and canonical values from oracle.cref.from_mont / f252_from_mont_limbs, never from the library."""
import ctypes
import functools
import hashlib
import json
import os
from collections import deque

import numpy as np
import pytest

from oracle import cref
from tests import backends, blake3_ref as b3
from tests.test_blake2s import _column, _row_bytes
from ministark_amd import (GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as F252, DeviceBytes, GpuVec, Matrix, MerkleTree,
                           grind_proof_of_work)
from ministark_amd._lib import MsError

HASH = "blake3_256"
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
WORDS = {FP: 1, FQ3: 3, F252: 4}
NAMES = {FP: "fp", FQ3: "fq3", F252: "fp252"}
KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blake3_kat.json")))


def _pattern(L):
    return bytes(i % 251 for i in range(L))


# ---- 1. the helper itself: scalar against the known answers, batched against scalar ---------------------------------------------------

def test_reference_matches_the_known_answers_and_its_batched_form():
    assert sorted(int(L) for L in KAT["by_length"]) == [0, 1, 63, 64, 65, 128, 1023, 1024, 1025, 2048, 2049, 3072, 3073, 4096]
    for L, want in KAT["by_length"].items():
        assert b3.blake3(_pattern(int(L))).hex() == want, L
    assert b3.blake3(b"abc").hex() == KAT["abc"]
    rng = np.random.default_rng(3)
    for L in (0, 1, 8, 40, 63, 64, 65, 1023, 1024, 1025, 1032, 2048, 2056, 3072, 3073, 3104, 4096):
        msgs = rng.integers(0, 256, size=(3, L), dtype=np.uint8)
        if L:
            msgs[0] = np.frombuffer(_pattern(L), dtype=np.uint8)
        got = b3.blake3_many(msgs)
        assert [got[i].tobytes() for i in range(3)] == [b3.blake3(msgs[i].tobytes()) for i in range(3)], L
    leaves = rng.integers(0, 256, size=(8, 32), dtype=np.uint8)
    nodes = b3.merkle_nodes(leaves)
    assert not nodes[0].any()
    for k in range(1, 8):
        left = leaves[2 * k - 8] if 2 * k >= 8 else nodes[2 * k]
        right = leaves[2 * k + 1 - 8] if 2 * k + 1 >= 8 else nodes[2 * k + 1]
        assert nodes[k].tobytes() == b3.blake3(left.tobytes() + right.tobytes()), k
    seed = bytes(range(32))
    n = 1
    while b3.leading_zero_bits(b3.blake3(seed + n.to_bytes(8, "big"))) < 7:
        n += 1
    assert b3.pow_search(seed, 7) == n and b3.pow_search(seed, 0) == 1


# ---- 2. rows at every block and chunk edge -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rows_inputs(field, ncols, nrows):
    """(columns, expected leaves as (nrows, 32) uint8): computed once, shared by the backends and left unchanged"""
    cols = [_column(field, nrows, 1000 * ncols + 17 * c + nrows) for c in range(ncols)]
    raw = np.frombuffer(b"".join(_row_bytes(field, cols, nrows)), dtype=np.uint8).reshape(nrows, ncols * WORDS[field] * 8)
    want = b3.blake3_many(raw)
    for a in cols:
        a.setflags(write=False)
    want.setflags(write=False)
    return cols, want


def _same_leaves(got, want, what):
    got = np.asarray(got).reshape(-1, 32)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: row {bad[0]} of {len(want)}"


# Fp: 8 columns a block, 128 columns exactly one chunk.  Fq3 (24 bytes): 43 columns put the first byte into chunk 1, 86 reach chunk 2,
# 128 are exactly three chunks.  Fp252 (32 bytes): 32 / 64 / 96 / 128 columns are exactly 1 / 2 / 3 / 4 chunks, 33 / 65 / 97 one element past.
ROW_CASES = ([(FP, c) for c in (1, 7, 8, 9, 16, 17, 127, 128)] + [(FQ3, c) for c in (1, 2, 3, 5, 6, 42, 43, 85, 86, 128)]
             + [(F252, c) for c in (1, 2, 3, 31, 32, 33, 64, 65, 96, 97, 128)])
ROW_IDS = [f"{NAMES[f]}-{c}" for f, c in ROW_CASES]
ROW_COUNTS = (5, 300)                       # ragged, and past one workgroup


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("field,ncols", ROW_CASES, ids=ROW_IDS)
def test_rows_block_and_chunk_edges(kind, field, ncols):
    pl = backends.planner(kind)
    for nrows in ROW_COUNTS:
        cols, want = _rows_inputs(field, ncols, nrows)
        got = Matrix.from_numpy(pl, [np.array(c) for c in cols], field).hash_rows(HASH).to_numpy()
        _same_leaves(got, want, f"{nrows} rows")


@pytest.mark.parametrize("kind", BACKENDS)
def test_rows_without_columns(kind):
    pl = backends.planner(kind)
    for nrows in ROW_COUNTS:
        leaves = DeviceBytes(pl, nrows * 32)
        pl.lib.check(pl.lib.ms_blake3_rows(pl.handle, FP, nrows, None, 0, leaves.ptr))
        assert leaves.to_numpy().tobytes() == bytes.fromhex(KAT["by_length"]["0"]) * nrows


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("ncols", [1, 9, 43, 128])
@pytest.mark.parametrize("field", [FP, FQ3, F252], ids=["fp", "fq3", "fp252"])
def test_rows_row_major(kind, field, ncols):
    """the row-major entry point is the same kernel with another stride: the de-interleaved matrix gives the same leaves"""
    pl = backends.planner(kind)
    V = WORDS[field]
    for nrows in ROW_COUNTS:
        cols, want = _rows_inputs(field, ncols, nrows)
        matrix = np.ascontiguousarray(np.stack([np.asarray(c).reshape(nrows, V) for c in cols], axis=1)).ravel()      # [row][column][word]
        d = GpuVec.from_numpy(pl, matrix, field)
        leaves = DeviceBytes(pl, nrows * 32)
        pl.lib.check(pl.lib.ms_blake3_rows_row_major(pl.handle, field, nrows, ncols, d.ptr, leaves.ptr))
        _same_leaves(leaves.to_numpy(), want, f"{nrows} rows")


@pytest.mark.parametrize("kind", BACKENDS)
def test_fri_layer_commitment(kind):
    pl = backends.planner(kind)
    n, ff = 1 << 9, 8
    ev = _column(FQ3, n, 55)
    tree = MerkleTree.from_fri_layer(GpuVec.from_numpy(pl, ev, FQ3), ff, HASH)
    rows = ev.reshape(n // ff, ff, 3)
    cols = [np.ascontiguousarray(rows[:, k, :]).ravel() for k in range(ff)]
    raw = np.frombuffer(b"".join(_row_bytes(FQ3, cols, n // ff)), dtype=np.uint8).reshape(n // ff, ff * 24)
    want = b3.blake3_many(raw)
    _same_leaves(tree.leaves.to_numpy(), want, "layer")
    assert tree.root() == b3.merkle_nodes(want)[1].tobytes()


# ---- 3. known answers through the C ABI --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", BACKENDS)
def test_known_answers(kind):
    """the bytes i % 251 are canonical as Goldilocks words: the top byte of every 8-byte word is at most 0xFA, so the word is below p"""
    pl = backends.planner(kind)
    for field, ncols in ((FP, 8), (FP, 16), (FP, 128), (FQ3, 128)):
        V = WORDS[field]
        L = ncols * V * 8
        words = np.frombuffer(_pattern(L), dtype="<u8").astype(np.uint64)
        assert int(words.max()) < cref.GL_P
        cols = [cref.to_mont(np.ascontiguousarray(words.reshape(ncols, V)[c])) for c in range(ncols)]
        got = Matrix.from_numpy(pl, cols, field).hash_rows(HASH).to_numpy().tobytes()
        assert got.hex() == KAT["by_length"][str(L)], (NAMES[field], ncols)
    leaves = DeviceBytes(pl, 32)
    pl.lib.check(pl.lib.ms_blake3_rows(pl.handle, FP, 1, None, 0, leaves.ptr))
    assert leaves.to_numpy().tobytes().hex() == KAT["by_length"]["0"]
    # a merge is the plain hash of 64 bytes: a two-leaf tree over the pattern has the L = 64 vector as its root
    lv = DeviceBytes(pl, 64)
    pl.lib.check(pl.lib.ms_upload(pl.handle, lv.ptr, _pattern(64), 64))
    tree = MerkleTree(pl, lv, 2, HASH)
    assert tree.root().hex() == KAT["by_length"]["64"]
    assert not tree.nodes_numpy()[0].any()


# ---- 4. trees: both sides of every level / subtree / top switch of the host schedule -----------------------------------------------

@functools.lru_cache(maxsize=None)
def _tree_inputs(log_n):
    n = 1 << log_n
    raw = np.random.default_rng(300 + log_n).integers(0, 256, size=(n, 32), dtype=np.uint8)
    nodes = b3.merkle_nodes(raw)
    raw.setflags(write=False)
    nodes.setflags(write=False)
    return raw, nodes


def _verify(root, view, indices):
    """MerkleTreeImpl::verify (src/merkle.rs:208-287) with H = BLAKE3: True iff the batched opening leads to `root`"""
    H = b3.blake3
    n = 1 << view["height"]
    idx = sorted(set(indices))
    siblings, nodes = deque(view["sibling_leaves"]), deque(view["nodes"])
    queue = deque()
    leaves = deque(zip(idx, view["initial_leaves"]))
    while leaves:
        i, leaf = leaves.popleft()
        if leaves and (i ^ 1) == leaves[0][0]:
            queue.append(((n + i) >> 1, H(leaf + leaves.popleft()[1])))
            continue
        s = siblings.popleft()
        queue.append(((n + i) >> 1, H(leaf + s) if i % 2 == 0 else H(s + leaf)))
    while queue:
        i, h = queue.popleft()
        if i == 1:
            return h == root
        if queue and (i ^ 1) == queue[0][0]:
            queue.append((i >> 1, H(h + queue.popleft()[1])))
            continue
        s = nodes.popleft()
        queue.append((i >> 1, H(h + s) if i % 2 == 0 else H(s + h)))
    return False


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("log_n", [1, 5, 9, 10, 13, 17, 18])
def test_tree_shapes(kind, log_n):
    pl = backends.planner(kind)
    n = 1 << log_n
    raw, want = _tree_inputs(log_n)
    lv = DeviceBytes(pl, n * 32)
    pl.lib.check(pl.lib.ms_upload(pl.handle, lv.ptr, raw.ctypes.data, n * 32))
    tree = MerkleTree(pl, lv, n, HASH)
    got = tree.nodes_numpy().reshape(n, 32)
    assert not got[0].any(), "nodes[0] must stay zero"
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"node {bad[0]}"
    assert tree.root() == want[1].tobytes()
    indices = sorted({0, n - 1, n // 2, min(n - 1, 3), min(n - 1, 4)})
    view = tree.prove(indices)
    assert view["initial_leaves"] == [raw[i].tobytes() for i in indices]
    assert _verify(tree.root(), view, indices)
    leaf = bytearray(view["initial_leaves"][0])
    leaf[5] ^= 0x10
    assert not _verify(tree.root(), dict(view, initial_leaves=[bytes(leaf)] + list(view["initial_leaves"][1:])), indices)


@pytest.mark.parametrize("kind", BACKENDS)
def test_matrix_tree_and_openings(kind):
    pl = backends.planner(kind)
    cols, want = _rows_inputs(FP, 9, 256)
    m = Matrix.from_numpy(pl, [np.array(c) for c in cols], FP)
    tree = MerkleTree.from_matrix(m, HASH)
    assert tree.root() == b3.merkle_nodes(want)[1].tobytes()
    for indices in ([0], [255], [3, 4, 5, 200], [1, 17, 18, 19, 100, 101, 254]):
        view = tree.prove(indices)
        assert view["initial_leaves"] == [want[i].tobytes() for i in sorted(set(indices))]
        assert _verify(tree.root(), view, indices)


# ---- 5. proof of work ------------------------------------------------------------------------------------------------------------

POW_SEEDS = [hashlib.sha256(bytes([s, 7])).digest() for s in range(2)]


@functools.lru_cache(maxsize=None)
def _pow_want(seed, bits):
    return b3.pow_search(seed, bits)


@pytest.mark.parametrize("kind", BACKENDS)
def test_pow_is_the_smallest_nonce(kind):
    pl = backends.planner(kind)
    for seed in POW_SEEDS:
        for bits in (0, 1, 9, 12):
            need = _pow_want(seed, bits)
            assert grind_proof_of_work(pl, seed, bits, 1 << 32, hash=HASH) == need, (seed.hex(), bits)
        need = _pow_want(seed, 9)
        assert need > 1
        with pytest.raises(MsError, match="no nonce below") as e:
            grind_proof_of_work(pl, seed, 9, need - 1, hash=HASH)
        assert e.value.code == -1
        assert grind_proof_of_work(pl, seed, 9, need, hash=HASH) == need
    with pytest.raises(MsError, match="bits must be <= 64") as e:
        grind_proof_of_work(pl, POW_SEEDS[0], 65, hash=HASH)
    assert e.value.code == -1
    # the other hashes grind as they did
    n = 1
    while b3.leading_zero_bits(hashlib.sha256(POW_SEEDS[0] + n.to_bytes(8, "big")).digest()) < 6:
        n += 1
    assert grind_proof_of_work(pl, POW_SEEDS[0], 6) == n


# ---- 6. refusals and names ---------------------------------------------------------------------------------------------------------

def test_error_paths_emu():
    pl = backends.planner("emu")
    L = pl.lib
    col = GpuVec.from_numpy(pl, cref.random_elements(8, 1))
    cols = (ctypes.c_void_p * 1)(col.ptr)
    out = DeviceBytes(pl, 8 * 32)
    out2 = DeviceBytes(pl, 8 * 32)
    seed = ctypes.create_string_buffer(32)
    nonce = ctypes.c_uint64(0)
    for rc in (L.ms_blake3_rows(None, FP, 8, cols, 1, out.ptr), L.ms_blake3_rows(pl.handle, FP, 8, None, 1, out.ptr),
               L.ms_blake3_rows(pl.handle, FP, 8, cols, 1, None), L.ms_blake3_rows(pl.handle, FP, 8, (ctypes.c_void_p * 1)(None), 1, out.ptr),
               L.ms_blake3_rows_row_major(pl.handle, FP, 8, 1, None, out.ptr), L.ms_blake3_rows_row_major(None, FP, 8, 1, col.ptr, out.ptr),
               L.ms_blake3_merkle(pl.handle, 8, None, out2.ptr), L.ms_blake3_merkle(pl.handle, 8, out.ptr, None),
               L.ms_blake3_pow_grind(pl.handle, None, 1, 10, ctypes.byref(nonce)), L.ms_blake3_pow_grind(pl.handle, seed, 1, 10, None)):
        assert rc == -1
    many = (ctypes.c_void_p * 129)(*([col.ptr] * 129))
    with pytest.raises(MsError, match="at most 128 columns") as e:
        L.check(L.ms_blake3_rows(pl.handle, FP, 8, many, 129, out.ptr))
    assert e.value.code == -2
    with pytest.raises(MsError, match="1..128 columns") as e:
        L.check(L.ms_blake3_rows_row_major(pl.handle, FP, 1, 129, col.ptr, out.ptr))
    assert e.value.code == -2
    with pytest.raises(MsError, match="1..128 columns") as e:
        L.check(L.ms_blake3_rows_row_major(pl.handle, FP, 1, 0, col.ptr, out.ptr))
    assert e.value.code == -2
    with pytest.raises(MsError, match="power of two"):
        L.check(L.ms_blake3_merkle(pl.handle, 3, out.ptr, out2.ptr))
    with pytest.raises(MsError, match="power of two"):
        L.check(L.ms_blake3_merkle(pl.handle, 1, out.ptr, out2.ptr))
    with pytest.raises(MsError, match="unknown field id 7"):
        L.check(L.ms_blake3_rows(pl.handle, 7, 8, cols, 1, out.ptr))
    with pytest.raises(MsError, match="unknown field id 9"):
        L.check(L.ms_blake3_rows_row_major(pl.handle, 9, 8, 1, col.ptr, out.ptr))
    assert L.ms_blake3_rows(pl.handle, FP, 0, cols, 1, out.ptr) == 0             # no rows: nothing to do


def test_names_emu():
    from ministark_amd import api
    pl = backends.planner("emu")
    col = GpuVec.from_numpy(pl, cref.random_elements(8, 1))
    assert HASH in api.HASHES and "blake3" not in api.HASHES
    assert api.pow_hash(HASH) == HASH and api.pow_hash("blake2s") == "blake2s" and api.pow_hash("rpo256") == "sha256"
    leaves = Matrix([col]).hash_rows(HASH)
    assert MerkleTree(pl, leaves, 8, HASH).root() == MerkleTree.from_matrix(Matrix([col]), HASH).root()
    assert grind_proof_of_work(pl, bytes(32), 3, hash=HASH) == _pow_want(bytes(32), 3)
    with pytest.raises(ValueError, match="unknown hash"):
        Matrix([col]).hash_rows("blake3")
    with pytest.raises(ValueError, match="unknown hash"):
        MerkleTree(pl, leaves, 8, "blake3")
    with pytest.raises(ValueError, match="unknown hash"):
        MerkleTree.from_fri_layer(col, 2, "blake3")
    with pytest.raises(ValueError, match="unknown proof-of-work hash"):
        grind_proof_of_work(pl, bytes(32), 1, hash="blake3")


@pytest.mark.parametrize("kind", BACKENDS)
def test_checked_mode_refuses_a_non_canonical_row_before_anything_is_written(kind):
    pl = backends.planner(kind)
    L = pl.lib
    nrows, ncols = 40, 3
    words = [cref.random_elements(nrows, 70 + c) for c in range(ncols)]
    words[1][17] = np.uint64(cref.GL_P)                                            # not a residue below p
    cols = [GpuVec.from_numpy(pl, w) for w in words]
    ptrs = (ctypes.c_void_p * ncols)(*[c.ptr for c in cols])
    rowmajor = GpuVec.from_numpy(pl, np.ascontiguousarray(np.stack(words, axis=1)).ravel())
    guard = bytes([0xAB]) * (nrows * 32)
    try:
        pl.checked(True)
        for entry, call in (("ms_blake3_rows", lambda out: L.ms_blake3_rows(pl.handle, FP, nrows, ptrs, ncols, out.ptr)),
                            ("ms_blake3_rows_row_major", lambda out: L.ms_blake3_rows_row_major(pl.handle, FP, nrows, ncols, rowmajor.ptr, out.ptr))):
            out = DeviceBytes(pl, nrows * 32)
            L.check(L.ms_upload(pl.handle, out.ptr, guard, len(guard)))
            assert call(out) == -1
            msg = L.ms_last_error().decode()
            assert "canonical" in msg and entry in msg and "column 1, row 17" in msg, msg
            assert out.to_numpy().tobytes() == guard, "a refused call wrote its output"
        pl.checked(False)
        out = DeviceBytes(pl, nrows * 32)
        assert L.ms_blake3_rows(pl.handle, FP, nrows, ptrs, ncols, out.ptr) == 0   # unchecked, the call is not refused
    finally:
        pl.checked(False)
