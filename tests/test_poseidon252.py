"""Starknet's Poseidon over the 252-bit field (ms_poseidon252_*, hash="poseidon252"): the simulator and the device against
tests/poseidon_ref.py -- Python integers from the recipe alone -- word for word, through the C ABI and the Python mirror.

The first test pins the helper to the known answers of the function (the first of them the published vector of the Starknet
implementation) before anything is compared with it.  Expected values are computed once per shape and shared by the two backends."""
import ctypes
import functools
import random
from collections import deque

import numpy as np
import pytest

from oracle import cref
from tests import backends, poseidon_ref as ref
from ministark_amd import (GOLDILOCKS_FP as FP, STARK252_FP as F252, DeviceBytes, GpuVec, Matrix, MerkleTree, poseidon252_permute,
                           poseidon252_value)
from ministark_amd._lib import MsError
from ministark_amd.api import HASHES, f252_from_mont_limbs

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
P = ref.P
EDGES = [0, 1, 2, P - 1, P - 2, (P - 1) // 2]
TOP = 256          # mspos::TOP: ms_poseidon252_merkle runs every level of at most 256 parents in one launch, one launch per level above
#                    that -- 2^9 leaves are the largest tree that is the top launch alone, 2^10 the first with a level launch in front


def words(values):
    """canonical integers -> the flat array of their Montgomery words"""
    return np.array([w for v in values for w in ref.to_words(v)], dtype=np.uint64)


def values(arr):
    return [ref.from_words(r) for r in np.asarray(arr, dtype=np.uint64).reshape(-1, 4)]


def digest_values(device_bytes):
    return values(device_bytes.to_numpy().view(np.uint64))


# ---- 0. the helper is pinned before anything is compared with it ------------------------------------------------------------------

def test_helper_is_pinned_to_the_known_answers():
    assert ref.RC[0] == 2950795762459345168613727575620414179244544320470208355568817838579231751791 and len(ref.RC) == 273
    assert ref.permute(0, 0, 0) == (3446325744004048536138401612021367625846492093718951375866996507163446763827,
                                    1590252087433376791875644726012779423683501236913937337746052470473806035332,
                                    867921192302518434283879514999422690776342565400001269945778456016268852423)
    assert ref.permute(P - 1, P - 1, P - 1)[0] == 0x5a5f2203787ca729e974a3156ebf02128c355cebc22cb6371c94c6d8eb1b78
    assert ref.hash2(1, 2) == 0x5d44a3decb2b2e0cc71071f7b802f45dd792d064f0fc7316c46514f70f9891a
    assert ref.hash2(P - 1, P - 1) == 0x8240c823e0ce7f8300da42d6a28931c23f7e2eec7dd8d7e4caae97f1fd28cf
    assert ref.hash_many([]) == 0x2272be0f580fd156823304800919530eaa97430e972d7213ee13f4fbf7a5dbc
    assert ref.hash_many([1]) == 0x579e8877c7755365d5ec1ec7d3a94a457eff5d1f40482bbe9729c064cdead2
    assert ref.hash_many([1, 2]) == 0x371cb6995ea5e7effcd2e174de264b5b407027a75a231a70c2c8d196107f0e7
    assert ref.hash_many([1, 2, 3]) == 0x2f0d8840bcf3bc629598d8a6cc80cb7c0d9e52d93dab244bbf9cd0dca0ad082
    assert ref.hash_many([]) == ref.permute(1, 0, 0)[0]
    for v in (0, 1, P - 1, 1234567 << 200):                                   # the word form and back, against the package's host-side conversion
        assert ref.from_words(ref.to_words(v)) == v
        assert f252_from_mont_limbs(np.array(ref.to_words(v), dtype=np.uint64)) == v
        assert poseidon252_value(ref.digest_bytes(v)) == v == ref.digest_value(ref.digest_bytes(v))
    assert "poseidon252" in HASHES


# ---- 1. the permutation -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _state_pool():
    """257 states: the three whose sums with the round-0 constants are exactly p, p - 1 and p + 1 in every element, {edges}^3, random ones"""
    rnd = random.Random(252)
    pool = [tuple(P - ref.RC[j] + d for j in range(3)) for d in (0, -1, 1)]
    pool += [(a, b, c) for a in EDGES for b in EDGES for c in EDGES]
    pool += [tuple(rnd.randrange(P) for _ in range(3)) for _ in range(257 - len(pool))]
    assert len(pool) == 257 and all(0 <= x < P for s in pool for x in s)
    assert [(pool[k][0] + ref.RC[0]) - P for k in range(3)] == [0, -1, 1]
    return pool, [ref.permute(*s) for s in pool]


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_permutation(kind, n):
    pl = backends.planner(kind)
    pool, want = _state_pool()
    pick = [(k * 5 + n) % 257 for k in range(n)] if n < 257 else list(range(257))        # every n starts somewhere else in the pool
    if n >= 63:
        pick[:3] = [0, 1, 2]                                                             # the round-0 carry edges
    states = GpuVec.from_numpy(pl, words([x for k in pick for x in pool[k]]), F252)
    out = poseidon252_permute(pl, states)
    got = values(out.to_numpy())
    assert [tuple(got[3 * i: 3 * i + 3]) for i in range(n)] == [want[k] for k in pick]
    assert np.array_equal(states.to_numpy(), words([x for k in pick for x in pool[k]]))   # the input is left alone
    pl.lib.check(pl.lib.ms_poseidon252_permute(pl.handle, n, states.ptr, states.ptr))    # in place
    assert np.array_equal(states.to_numpy(), out.to_numpy())


@pytest.mark.parametrize("kind", BACKENDS)
def test_known_answers_on_the_device(kind):
    pl = backends.planner(kind)
    out = values(poseidon252_permute(pl, GpuVec.from_numpy(pl, words([0, 0, 0, 1, 2, 2, P - 1, P - 1, P - 1]), F252)).to_numpy())
    assert tuple(out[:3]) == ref.permute(0, 0, 0)
    assert out[3] == 0x5d44a3decb2b2e0cc71071f7b802f45dd792d064f0fc7316c46514f70f9891a
    assert out[6] == 0x5a5f2203787ca729e974a3156ebf02128c355cebc22cb6371c94c6d8eb1b78
    one = Matrix.from_numpy(pl, [words([1]), words([2]), words([3])], F252)
    assert digest_values(one.hash_rows("poseidon252")) == [0x2f0d8840bcf3bc629598d8a6cc80cb7c0d9e52d93dab244bbf9cd0dca0ad082]
    lv = DeviceBytes(pl, 64)
    pl.lib.check(pl.lib.ms_upload(pl.handle, lv.ptr, ref.digest_bytes(P - 1) * 2, 64))
    assert poseidon252_value(MerkleTree(pl, lv, 2, "poseidon252").root()) == 0x8240c823e0ce7f8300da42d6a28931c23f7e2eec7dd8d7e4caae97f1fd28cf


# ---- 2. the sponge over rows --------------------------------------------------------------------------------------------------------

MAXROWS = 257                                                  # one full workgroup and a ragged one


@functools.lru_cache(maxsize=None)
def _column(seed, n=MAXROWS):
    """n canonical integers: the edge elements in the first rows (rotated by the seed), random ones after"""
    rnd = random.Random(seed)
    col = [rnd.randrange(P) for _ in range(n)]
    for k, e in enumerate(EDGES[: min(n, len(EDGES))]):
        col[(k + seed) % min(n, 8)] = e
    return col


@functools.lru_cache(maxsize=None)
def _want_leaves(ncols, seed):
    cols = [_column(seed + 17 * c) for c in range(ncols)]
    return [ref.hash_many([c[r] for c in cols]) for r in range(MAXROWS)]


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("ncols", [0, 1, 2, 3, 7, 8, 9, 127, 128])
def test_rows(kind, ncols):
    """hash_many over the first nrows rows of the same columns, every nrows with every ncols: the expected leaves are computed once for
    257 rows and shared by the two backends (the widest rows, 64 and 65 absorbs each, are 3.7 s of reference)"""
    pl = backends.planner(kind)
    seed = 300 + ncols
    want = _want_leaves(ncols, seed)
    for nrows in (1, 64, 65, 257):
        vecs = [GpuVec.from_numpy(pl, words(_column(seed + 17 * c)[:nrows]), F252) for c in range(ncols)]
        ptrs = (ctypes.c_void_p * max(1, ncols))(*[v.ptr for v in vecs])
        leaves = DeviceBytes(pl, nrows * 32)
        pl.lib.check(pl.lib.ms_poseidon252_rows(pl.handle, nrows, ptrs if ncols else None, ncols, leaves.ptr))
        assert digest_values(leaves) == want[:nrows], nrows
        if ncols:                                              # the name-selected path gives the same leaves
            assert np.array_equal(Matrix(vecs).hash_rows("poseidon252").to_numpy(), leaves.to_numpy())
    if ncols == 0:
        assert set(want) == {0x2272be0f580fd156823304800919530eaa97430e972d7213ee13f4fbf7a5dbc}
        pl.lib.check(pl.lib.ms_poseidon252_rows(pl.handle, 0, None, 0, leaves.ptr))      # no rows: nothing happens


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("ff", [2, 4, 8, 16])
def test_fri_layer_rows(kind, ff):
    pl = backends.planner(kind)
    seed = 500 + ff
    want = _want_leaves(ff, seed)
    cols = [_column(seed + 17 * c) for c in range(ff)]
    for nrows in (1, 64, 65, 257):
        layer = GpuVec.from_numpy(pl, words([cols[c][r] for r in range(nrows) for c in range(ff)]), F252)      # row r = ff consecutive elements
        leaves = DeviceBytes(pl, nrows * 32)
        pl.lib.check(pl.lib.ms_poseidon252_rows_row_major(pl.handle, nrows, ff, layer.ptr, leaves.ptr))
        assert digest_values(leaves) == want[:nrows]
    # MerkleTree.from_fri_layer over a power-of-two layer takes the same path
    layer = GpuVec.from_numpy(pl, words([cols[c][r] for r in range(64) for c in range(ff)]), F252)
    tree = MerkleTree.from_fri_layer(layer, ff, "poseidon252")
    assert digest_values(tree.leaves) == want[:64]
    _check_tree(tree, want[:64])


# ---- 3. trees ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tree(log_n):
    rnd = random.Random(1000 + log_n)
    leaves = [rnd.randrange(P) for _ in range(1 << log_n)]
    for k, e in enumerate(EDGES[: len(leaves)]):
        leaves[-1 - k] = e
    return leaves, ref.merkle_nodes(leaves)


def _check_tree(tree, leaves, want=None):
    want = want or ref.merkle_nodes(leaves)
    raw = tree.nodes_numpy()
    assert not raw[0].any(), "nodes[0] must stay zero"
    got = values(raw.view(np.uint64))
    bad = [k for k in range(1, len(leaves)) if got[k] != want[k]]
    assert not bad, f"nodes {bad[:8]}"
    assert poseidon252_value(tree.root()) == want[1]


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("log_n", range(1, 14))
def test_tree_every_node(kind, log_n):
    """2^1 .. 2^13 leaves: up to 2^9 the top launch alone (TOP = 256 parents), from 2^10 one level launch per level above it"""
    assert TOP == 256
    pl = backends.planner(kind)
    leaves, want = _tree(log_n)
    n = len(leaves)
    lv = DeviceBytes(pl, n * 32)
    raw = words(leaves)
    pl.lib.check(pl.lib.ms_upload(pl.handle, lv.ptr, raw.ctypes.data, n * 32))
    _check_tree(MerkleTree(pl, lv, n, "poseidon252"), leaves, want)


@pytest.mark.parametrize("kind", BACKENDS)
def test_tree_over_hashed_rows_and_its_openings(kind):
    pl = backends.planner(kind)
    n, ncols, seed = 256, 3, 700
    m = Matrix.from_numpy(pl, [words(_column(seed + 17 * c)[:n]) for c in range(ncols)], F252)
    leaves = _want_leaves(ncols, seed)[:n]
    tree = MerkleTree.from_matrix(m, "poseidon252")
    assert digest_values(tree.leaves) == leaves
    _check_tree(tree, leaves)
    root = poseidon252_value(tree.root())
    # duplicate positions, adjacent positions, the first leaf and the last leaf
    for indices in ([0], [n - 1], [0, n - 1], [7, 7, 7], [4, 5], [5, 6], [3, 4, 5, 200, 200], [1, 17, 18, 19, 100, 101, 254, 255, 0]):
        view = tree.prove(indices)
        assert [poseidon252_value(d) for d in view["initial_leaves"]] == [leaves[i] for i in sorted(set(indices))]
        assert _verify(root, view, indices)
        bad = dict(view, initial_leaves=list(view["initial_leaves"]))
        bad["initial_leaves"][0] = ref.digest_bytes((poseidon252_value(bad["initial_leaves"][0]) + 1) % P)
        assert not _verify(root, bad, indices)


def _verify(root, view, indices):
    """MerkleTreeImpl::verify with H = hash2 over the digests' integers: True iff the batched opening leads to `root`"""
    val = poseidon252_value
    n = 1 << view["height"]
    idx = sorted(set(indices))
    siblings, nodes = deque(val(d) for d in view["sibling_leaves"]), deque(val(d) for d in view["nodes"])
    queue = deque()
    leaves = deque(zip(idx, [val(d) for d in view["initial_leaves"]]))
    while leaves:
        i, leaf = leaves.popleft()
        if leaves and (i ^ 1) == leaves[0][0]:
            queue.append(((n + i) >> 1, ref.hash2(leaf, leaves.popleft()[1])))
            continue
        s = siblings.popleft()
        queue.append(((n + i) >> 1, ref.hash2(leaf, s) if i % 2 == 0 else ref.hash2(s, leaf)))
    while queue:
        i, d = queue.popleft()
        if i == 1:
            return d == root
        if queue and (i ^ 1) == queue[0][0]:
            queue.append((i >> 1, ref.hash2(d, queue.popleft()[1])))
            continue
        s = nodes.popleft()
        queue.append((i >> 1, ref.hash2(d, s) if i % 2 == 0 else ref.hash2(s, d)))
    return False


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_emu():
    pl = backends.planner("emu")
    L = pl.lib
    n = 8
    col = GpuVec.from_numpy(pl, words(_column(1)[:n]), F252)
    cols = (ctypes.c_void_p * 1)(col.ptr)
    out = DeviceBytes(pl, n * 96)
    before = out.to_numpy().copy()
    for rc in (L.ms_poseidon252_rows(None, n, cols, 1, out.ptr), L.ms_poseidon252_rows(pl.handle, n, None, 1, out.ptr),
               L.ms_poseidon252_rows(pl.handle, n, cols, 1, None),
               L.ms_poseidon252_rows_row_major(None, n, 1, col.ptr, out.ptr), L.ms_poseidon252_rows_row_major(pl.handle, n, 1, None, out.ptr),
               L.ms_poseidon252_rows_row_major(pl.handle, n, 1, col.ptr, None),
               L.ms_poseidon252_merkle(None, n, col.ptr, out.ptr), L.ms_poseidon252_merkle(pl.handle, n, None, out.ptr),
               L.ms_poseidon252_merkle(pl.handle, n, col.ptr, None),
               L.ms_poseidon252_permute(None, 2, col.ptr, out.ptr), L.ms_poseidon252_permute(pl.handle, 2, None, out.ptr),
               L.ms_poseidon252_permute(pl.handle, 2, col.ptr, None)):
        assert rc == -1
    with pytest.raises(MsError, match="null column 1") as e:
        L.check(L.ms_poseidon252_rows(pl.handle, n, (ctypes.c_void_p * 2)(col.ptr, None), 2, out.ptr))
    assert e.value.code == -1
    many = (ctypes.c_void_p * 129)(*([col.ptr] * 129))
    with pytest.raises(MsError, match="at most 128 columns") as e:
        L.check(L.ms_poseidon252_rows(pl.handle, n, many, 129, out.ptr))
    assert e.value.code == -2
    for ncols in (0, 129):
        with pytest.raises(MsError, match="1..128 columns") as e:
            L.check(L.ms_poseidon252_rows_row_major(pl.handle, 1, ncols, col.ptr, out.ptr))
        assert e.value.code == -2
    for nleaves in (3, 1, 0, 6):
        with pytest.raises(MsError, match="power of two") as e:
            L.check(L.ms_poseidon252_merkle(pl.handle, nleaves, col.ptr, out.ptr))
        assert e.value.code == -1
    # d_out == d_in is allowed (test_permutation); any other overlap is not: one state further, one word further, from behind
    big = GpuVec.from_numpy(pl, words(_column(2)[:12]), F252)               # four states
    for delta in (96, 8, -96):
        src, dst = (big.ptr, big.ptr + delta) if delta > 0 else (big.ptr - delta, big.ptr)
        with pytest.raises(MsError, match="overlap") as e:
            L.check(L.ms_poseidon252_permute(pl.handle, 2, src, dst))
        assert e.value.code == -1
    assert np.array_equal(big.to_numpy(), words(_column(2)[:12]))
    L.check(L.ms_poseidon252_permute(pl.handle, 2, big.ptr, big.ptr + 192))   # adjacent ranges do not overlap
    assert np.array_equal(out.to_numpy(), before)                           # every refusal came before anything was enqueued
    # the Python mirror: Poseidon is for the 252-bit field
    gl = Matrix.from_numpy(pl, [cref.random_elements(8, 1)], FP)
    with pytest.raises(ValueError, match="252-bit field"):
        gl.hash_rows("poseidon252")
    with pytest.raises(ValueError, match="252-bit field"):
        MerkleTree.from_matrix(gl, "poseidon252")
    with pytest.raises(ValueError, match="252-bit field"):
        MerkleTree.from_fri_layer(GpuVec.from_numpy(pl, cref.random_elements(16, 2), FP), 2, "poseidon252")
    with pytest.raises(ValueError, match="STARK252_FP"):
        poseidon252_permute(pl, GpuVec.from_numpy(pl, cref.random_elements(3, 2), FP))
    with pytest.raises(ValueError, match="unknown hash"):
        gl.hash_rows("poseidon")


@pytest.mark.parametrize("kind", BACKENDS)
def test_checked_mode_refuses_non_canonical_input(kind):
    """one word pattern >= p in a column, in a leaf and in a state: the error names the entry point, the argument and the place; the
    outputs are untouched; with the mode off the same calls are not refused"""
    pl = backends.planner(kind)
    L = pl.lib
    n = 16
    p_words = [(P >> (64 * k)) & ((1 << 64) - 1) for k in range(4)]          # the element p itself: every word in range, the value not
    top = [0, 0, 0, 1 << 63]                                                 # one word (the top one) far beyond p's

    def poisoned(count, row, bad):
        w = words(_column(40)[:count]).copy()
        w[4 * row: 4 * row + 4] = bad
        return w
    cases = []
    c0, c1 = GpuVec.from_numpy(pl, words(_column(41)[:n]), F252), GpuVec.from_numpy(pl, poisoned(n, 9, p_words), F252)
    ptrs = (ctypes.c_void_p * 2)(c0.ptr, c1.ptr)
    cases.append(("ms_poseidon252_rows: d_cols", r"column 1, row 9", lambda o: L.ms_poseidon252_rows(pl.handle, n, ptrs, 2, o.ptr), n * 32))
    mat = GpuVec.from_numpy(pl, poisoned(n * 4, 4 * 5 + 2, top), F252)
    cases.append(("ms_poseidon252_rows_row_major: d_matrix", r"column 2, row 5", lambda o: L.ms_poseidon252_rows_row_major(pl.handle, n, 4, mat.ptr, o.ptr), n * 32))
    lv = GpuVec.from_numpy(pl, poisoned(n, 7, p_words), F252)
    cases.append(("ms_poseidon252_merkle: d_leaves", r"column 0, row 7", lambda o: L.ms_poseidon252_merkle(pl.handle, n, lv.ptr, o.ptr), n * 32))
    st = GpuVec.from_numpy(pl, poisoned(n * 3, 3 * 6 + 1, top), F252)
    cases.append(("ms_poseidon252_permute: d_in", r"column 1, row 6", lambda o: L.ms_poseidon252_permute(pl.handle, n, st.ptr, o.ptr), n * 96))
    for where, place, call, nbytes in cases:
        out = DeviceBytes(pl, nbytes)
        L.check(L.ms_upload(pl.handle, out.ptr, bytes([0xA5]) * nbytes, nbytes))
        pl.checked(True)
        try:
            with pytest.raises(MsError, match=where + r" holds an element that is not canonical.*" + place) as e:
                L.check(call(out))
            assert e.value.code == -1
            assert set(out.to_numpy().tolist()) == {0xA5}, "the output must be untouched"
        finally:
            pl.checked(False)
        L.check(call(out))                                                   # checked mode off: not refused
        assert set(out.to_numpy().tolist()) != {0xA5}
