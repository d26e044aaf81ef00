"""BLAKE2s-256 commitments and proof-of-work (ms_blake2s_*, hash="blake2s"): device against hashlib.blake2s, byte-exact.

H = unkeyed BLAKE2s with a 32-byte digest.  Leaf of row r = H(canonical little-endian bytes of every element of the row), the bytes
the SHA-256 leaves hash (Fp 8 bytes, Fq3 c0||c1||c2, Fp252 32 bytes); nodes[k] = H(nodes[2k] || nodes[2k+1]); the nonce is the
smallest n >= 1 with `bits` leading zero bits of H(seed || n as 8 big-endian bytes).  Expected values come from hashlib here and
canonical values from oracle.cref.from_mont / f252_from_mont_limbs, never from the library."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import cref
from tests import backends
from ministark_amd import (GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as F252, DeviceBytes, GpuVec, Matrix, MerkleTree,
                           f252_from_mont_limbs, f252_to_mont_limbs, grind_proof_of_work)
from ministark_amd._lib import MsError

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
WORDS = {FP: 1, FQ3: 3, F252: 4}
P = cref.GL_P


def b2(data):
    return hashlib.blake2s(data).digest()


def _lz(d):
    z = 0
    for b in d:
        if b:
            return z + 8 - b.bit_length()
        z += 8
    return z


def _pow_search(seed, bits):
    n = 1
    while _lz(b2(seed + n.to_bytes(8, "big"))) < bits:
        n += 1
    return n


# ---- inputs: random Montgomery words plus the edge words, and their canonical bytes -----------------------------------------------

GL_EDGES = [0, 1, 2, P - 1, P - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63), P - (1 << 32)]


def _gl_words(n, seed):
    """n Goldilocks Montgomery words: random, with the edge values (as canonical values, converted to Montgomery form) up front"""
    w = cref.random_elements(n, seed)
    edges = cref.to_mont(np.array(GL_EDGES, dtype=np.uint64))
    k = min(n, len(edges))
    w[:k] = np.roll(edges, seed % len(edges))[:k]
    return w


def _f252_words(n, seed):
    rng = np.random.default_rng(seed)
    vals = [int.from_bytes(rng.bytes(32), "little") % cref.F252_P for _ in range(n)]
    edges = [0, 1, 2, cref.F252_P - 1, cref.F252_P - 2, 1 << 32, (1 << 64) - 1, 1 << 64, (1 << 192) - 1, 1 << 250]
    for i in range(min(n, len(edges))):
        vals[i] = edges[(i + seed) % len(edges)]
    return np.concatenate([f252_to_mont_limbs(v) for v in vals]) if n else np.zeros(0, np.uint64)


def _column(field, n, seed):
    if field == F252:
        return _f252_words(n, seed)
    return _gl_words(n * WORDS[field], seed)


def _row_bytes(field, cols, n):
    """canonical little-endian bytes of every row: list of n bytes objects"""
    V = WORDS[field]
    parts = []
    for c in cols:
        if field == F252:
            limbs = np.asarray(c).reshape(n, 4)
            parts.append([f252_from_mont_limbs(limbs[r]).to_bytes(32, "little") for r in range(n)])
        else:
            can = cref.from_mont(np.asarray(c)).astype("<u8").reshape(n, V)
            parts.append([can[r].tobytes() for r in range(n)])
    return [b"".join(p[r] for p in parts) for r in range(n)]


def _want_leaves(field, cols, n):
    return [b2(x) for x in _row_bytes(field, cols, n)]


def _want_nodes(leaves):
    n = len(leaves)
    nodes = [b""] * n
    nodes[0] = bytes(32)
    for k in range(n - 1, 0, -1):
        left = leaves[2 * k - n] if 2 * k >= n else nodes[2 * k]
        right = leaves[2 * k + 1 - n] if 2 * k + 1 >= n else nodes[2 * k + 1]
        nodes[k] = b2(left + right)
    return nodes


def _check_tree(tree, leaves):
    got = tree.nodes_numpy()
    want = _want_nodes(leaves)
    assert not got[0].any(), "nodes[0] must stay zero"
    for k in range(1, len(leaves)):
        assert got[k].tobytes() == want[k], f"node {k}"
    assert tree.root() == want[1]


# ---- 1. known answers --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", BACKENDS)
def test_known_answers(kind):
    pl = backends.planner(kind)
    one = Matrix.from_numpy(pl, [cref.to_mont(np.array([1], dtype=np.uint64))])
    assert one.hash_rows("blake2s").to_numpy().tobytes() == b2((1).to_bytes(8, "little"))
    assert one.hash_rows("blake2s").to_numpy().tobytes() == bytes.fromhex(
        hashlib.blake2s(bytes([1, 0, 0, 0, 0, 0, 0, 0])).hexdigest())
    # no columns: H(""), one zero block with counter 0
    leaves = DeviceBytes(pl, 4 * 32)
    pl.lib.check(pl.lib.ms_blake2s_rows(pl.handle, FP, 4, None, 0, leaves.ptr))
    assert all(leaves.to_numpy().reshape(4, 32)[r].tobytes() == b2(b"") for r in range(4))
    assert b2(b"").hex() == "69217a3079908094e11121d042354a7c1f55b6482ca1a51e1b250dfd1ed0eef9"
    # a merge of two fixed digests
    a, b = hashlib.sha256(b"left").digest(), hashlib.sha256(b"right").digest()
    lv = DeviceBytes(pl, 64)
    pl.lib.check(pl.lib.ms_upload(pl.handle, lv.ptr, a + b, 64))
    tree = MerkleTree(pl, lv, 2, "blake2s")
    assert tree.root() == b2(a + b)
    # a fixed proof-of-work nonce
    seed = bytes(range(32))
    assert grind_proof_of_work(pl, seed, 8, hash="blake2s") == _pow_search(seed, 8)


# ---- 2. rows at every block edge -------------------------------------------------------------------------------------------------

def _rows_case(kind, field, ncols, log_rows, seed):
    pl = backends.planner(kind)
    n = 1 << log_rows
    cols = [_column(field, n, seed + 17 * c) for c in range(ncols)]
    m = Matrix.from_numpy(pl, cols, field)
    got = m.hash_rows("blake2s").to_numpy().reshape(n, 32)
    want = _want_leaves(field, cols, n)
    for r in range(n):
        assert got[r].tobytes() == want[r], f"row {r}"
    return m, want


ROW_CASES = [(FP, c) for c in (1, 7, 8, 9, 16, 17, 128)] + [(FQ3, c) for c in (1, 2, 3, 6)] + [(F252, c) for c in (1, 2, 3, 4)]


@pytest.mark.parametrize("field,ncols", ROW_CASES)
def test_rows_block_edges_emu(field, ncols):
    _rows_case("emu", field, ncols, 5, 101 + ncols)


@pytest.mark.gpu
@pytest.mark.parametrize("field,ncols", ROW_CASES)
def test_rows_block_edges_hip(field, ncols):
    _rows_case("hip", field, ncols, 10, 201 + ncols)


# ---- 3. row-major FRI layers -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("field", [FP, FQ3, F252])
@pytest.mark.parametrize("ff", [2, 4, 8, 16])
def test_fri_layer_rows(kind, field, ff):
    pl = backends.planner(kind)
    V = WORDS[field]
    n = 1 << (8 if kind == "emu" else 12)
    ev = _column(field, n, 31 + ff)
    tree = MerkleTree.from_fri_layer(GpuVec.from_numpy(pl, ev, field), ff, "blake2s")
    rows = ev.reshape(n // ff, ff, V)
    cols = [np.ascontiguousarray(rows[:, k, :]).ravel() for k in range(ff)]           # the de-interleaved layer
    want = _want_leaves(field, cols, n // ff)
    assert [x.tobytes() for x in tree.leaves.to_numpy().reshape(n // ff, 32)] == want
    col_major = Matrix.from_numpy(pl, cols, field).hash_rows("blake2s").to_numpy()
    assert np.array_equal(tree.leaves.to_numpy(), col_major)
    _check_tree(tree, want)


# ---- 4. trees: every shape of the level / top split -------------------------------------------------------------------------------

def _tree_case(kind, log_n):
    pl = backends.planner(kind)
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    raw = rng.integers(0, 256, size=n * 32, dtype=np.uint8)
    lv = DeviceBytes(pl, n * 32)
    pl.lib.check(pl.lib.ms_upload(pl.handle, lv.ptr, raw.ctypes.data, n * 32))
    tree = MerkleTree(pl, lv, n, "blake2s")
    _check_tree(tree, [raw[32 * i: 32 * i + 32].tobytes() for i in range(n)])


@pytest.mark.parametrize("log_n", list(range(1, 11)) + [12, 17, 18])
def test_tree_shapes_emu(log_n):
    _tree_case("emu", log_n)


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [1, 5, 9, 10, 13, 17, 18, 19, 20, 21, 22])
def test_tree_shapes_hip(log_n):
    _tree_case("hip", log_n)


# ---- 5. openings ------------------------------------------------------------------------------------------------------------------

def _verify(root, view, indices):
    """MerkleTreeImpl::verify (src/merkle.rs:208-287) with H = BLAKE2s: True iff the batched opening leads to `root`"""
    from collections import deque
    n = 1 << view["height"]
    idx = sorted(set(indices))
    siblings, nodes = deque(view["sibling_leaves"]), deque(view["nodes"])
    queue = deque()
    leaves = deque(zip(idx, view["initial_leaves"]))
    while leaves:
        i, leaf = leaves.popleft()
        if leaves and (i ^ 1) == leaves[0][0]:
            queue.append(((n + i) >> 1, b2(leaf + leaves.popleft()[1])))
            continue
        s = siblings.popleft()
        queue.append(((n + i) >> 1, b2(leaf + s) if i % 2 == 0 else b2(s + leaf)))
    while queue:
        i, h = queue.popleft()
        if i == 1:
            return h == root
        if queue and (i ^ 1) == queue[0][0]:
            queue.append((i >> 1, b2(h + queue.popleft()[1])))
            continue
        s = nodes.popleft()
        queue.append((i >> 1, b2(h + s) if i % 2 == 0 else b2(s + h)))
    return False


@pytest.mark.parametrize("kind", BACKENDS)
def test_openings_verify_against_the_root(kind):
    m, want = _rows_case(kind, FP, 9, 8, 77)
    tree = MerkleTree.from_matrix(m, "blake2s")
    root = tree.root()
    for indices in ([0], [255], [3, 4, 5, 200], [1, 17, 18, 19, 100, 101, 254]):
        view = tree.prove(indices)
        assert view["initial_leaves"] == [want[i] for i in sorted(set(indices))]
        assert _verify(root, view, indices)
        bad = dict(view, initial_leaves=list(view["initial_leaves"]))
        leaf = bytearray(bad["initial_leaves"][0])
        leaf[5] ^= 0x10
        bad["initial_leaves"][0] = bytes(leaf)
        assert not _verify(root, bad, indices)


# ---- 6. proof of work ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", BACKENDS)
def test_pow_matches_linear_search(kind):
    pl = backends.planner(kind)
    top = 14 if kind == "hip" else 10
    for s in range(3):
        seed = hashlib.sha256(bytes([s, 7])).digest()
        for bits in range(0, top + 1, 1 if kind == "hip" else 2):
            assert grind_proof_of_work(pl, seed, bits, 1 << 32, hash="blake2s") == _pow_search(seed, bits), (s, bits)
    # the default is still SHA-256
    seed = hashlib.sha256(b"default").digest()
    n = 1
    while _lz(hashlib.sha256(seed + n.to_bytes(8, "big")).digest()) < 6:
        n += 1
    assert grind_proof_of_work(pl, seed, 6) == n


def test_pow_errors_emu():
    pl = backends.planner("emu")
    seed = hashlib.sha256(b"e").digest()
    with pytest.raises(MsError, match="bits must be <= 64") as e:
        grind_proof_of_work(pl, seed, 65, hash="blake2s")
    assert e.value.code == -1
    need = _pow_search(seed, 9)
    with pytest.raises(MsError, match="no nonce below") as e:
        grind_proof_of_work(pl, seed, 9, need - 1, hash="blake2s")
    assert e.value.code == -1
    assert grind_proof_of_work(pl, seed, 9, need, hash="blake2s") == need
    with pytest.raises(ValueError, match="unknown proof-of-work hash"):
        grind_proof_of_work(pl, seed, 1, hash="rpo256")


# ---- 7. error paths --------------------------------------------------------------------------------------------------------------

def test_error_paths_emu():
    pl = backends.planner("emu")
    L = pl.lib
    col = GpuVec.from_numpy(pl, cref.random_elements(8, 1))
    cols = (ctypes.c_void_p * 1)(col.ptr)
    out = DeviceBytes(pl, 8 * 32)
    out2 = DeviceBytes(pl, 8 * 32)
    seed = ctypes.create_string_buffer(32)
    nonce = ctypes.c_uint64(0)
    for rc in (L.ms_blake2s_rows(None, FP, 8, cols, 1, out.ptr), L.ms_blake2s_rows(pl.handle, FP, 8, None, 1, out.ptr),
               L.ms_blake2s_rows(pl.handle, FP, 8, cols, 1, None), L.ms_blake2s_rows(pl.handle, FP, 8, (ctypes.c_void_p * 1)(None), 1, out.ptr),
               L.ms_blake2s_rows_row_major(pl.handle, FP, 8, 1, None, out.ptr), L.ms_blake2s_rows_row_major(None, FP, 8, 1, col.ptr, out.ptr),
               L.ms_blake2s_merkle(pl.handle, 8, None, out2.ptr), L.ms_blake2s_merkle(pl.handle, 8, out.ptr, None),
               L.ms_blake2s_pow_grind(pl.handle, None, 1, 10, ctypes.byref(nonce)), L.ms_blake2s_pow_grind(pl.handle, seed, 1, 10, None)):
        assert rc == -1
    many = (ctypes.c_void_p * 129)(*([col.ptr] * 129))
    with pytest.raises(MsError, match="at most 128 columns") as e:
        L.check(L.ms_blake2s_rows(pl.handle, FP, 8, many, 129, out.ptr))
    assert e.value.code == -2
    with pytest.raises(MsError, match="1..128 columns") as e:
        L.check(L.ms_blake2s_rows_row_major(pl.handle, FP, 1, 129, col.ptr, out.ptr))
    assert e.value.code == -2
    with pytest.raises(MsError, match="power of two"):
        L.check(L.ms_blake2s_merkle(pl.handle, 3, out.ptr, out2.ptr))
    with pytest.raises(MsError, match="power of two"):
        L.check(L.ms_blake2s_merkle(pl.handle, 1, out.ptr, out2.ptr))
    with pytest.raises(MsError, match="unknown field id 7"):
        L.check(L.ms_blake2s_rows(pl.handle, 7, 8, cols, 1, out.ptr))
    with pytest.raises(MsError, match="unknown field id 9"):
        L.check(L.ms_blake2s_rows_row_major(pl.handle, 9, 8, 1, col.ptr, out.ptr))
    with pytest.raises(ValueError, match="unknown hash"):
        Matrix([col]).hash_rows("blake3")
