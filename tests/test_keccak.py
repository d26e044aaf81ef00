"""Keccak-256 and SHA3-256 commitments and proof-of-work (ms_keccak_*, hash="keccak256" / "sha3_256"): device against
tests/keccak_ref.py and hashlib.sha3_256, byte-exact, through the C ABI.

H = the Keccak sponge (rate 136, domain byte 0x01 / 0x06).  Leaf of row r = H(canonical little-endian bytes of every element of the row),
the bytes the SHA-256 and BLAKE2s leaves hash; nodes[k] = H(nodes[2k] || nodes[2k+1]); the nonce is the smallest n >= 1 with `bits`
leading zero bits of H(seed || n as 8 big-endian bytes).  SHA3-256 expected values always come from hashlib, never from the helper;
Keccak-256 ones from the helper, which the first test pins to hashlib (0x06) and to the published Keccak-256 digests (0x01) before
anything is compared with it.  Canonical values come from oracle.cref.from_mont / f252_from_mont_limbs, never from the library."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import cref
from tests import backends, keccak_ref
from tests.test_blake2s import GL_EDGES, _column, _row_bytes, _lz  # noqa: F401  (the edge words and canonical row bytes of the twin's tests)
from ministark_amd import (GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as F252, DeviceBytes, GpuVec, Matrix, MerkleTree,
                           grind_proof_of_work)
from ministark_amd._lib import MsError

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
VARIANTS = ["keccak256", "sha3_256"]
VARIANT_ID = {"keccak256": 0, "sha3_256": 1}
WORDS = {FP: 1, FQ3: 3, F252: 4}
KECCAK_EMPTY = "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
KECCAK_ABC = "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


def h1(variant, data):
    """one digest: hashlib for SHA3-256, the pinned helper for Keccak-256"""
    return hashlib.sha3_256(data).digest() if variant == "sha3_256" else keccak_ref.keccak256(data)


def hmany(variant, msgs):
    """digests of equal-length messages"""
    if variant == "sha3_256":
        return [hashlib.sha3_256(m).digest() for m in msgs]
    return keccak_ref.sponge256_many(msgs, 0x01)


# ---- 0. the helper is pinned before anything is compared with it ------------------------------------------------------------------

def test_helper_is_pinned_to_hashlib_and_published_digests():
    rng = np.random.default_rng(1)
    for n in (0, 1, 64, 135, 136, 137, 271, 272, 273, 1000):
        data = bytes(rng.bytes(n))
        assert keccak_ref.sponge256(data, 0x06) == hashlib.sha3_256(data).digest(), n
        batch = [bytes(rng.bytes(n)) for _ in range(3)]
        assert keccak_ref.sponge256_many(batch, 0x06) == [hashlib.sha3_256(m).digest() for m in batch], n
        assert keccak_ref.sponge256_many(batch, 0x01) == [keccak_ref.sponge256(m, 0x01) for m in batch], n
    assert keccak_ref.sponge256(b"", 0x01).hex() == KECCAK_EMPTY
    assert keccak_ref.sponge256(b"abc", 0x01).hex() == KECCAK_ABC
    assert keccak_ref.H("keccak256", b"abc").hex() == KECCAK_ABC and keccak_ref.H("sha3_256", b"abc") == hashlib.sha3_256(b"abc").digest()
    with pytest.raises(KeyError):
        keccak_ref.H("blake2s", b"")                          # nothing falls back


# ---- 1. known answers --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", BACKENDS)
def test_known_answers(kind):
    pl = backends.planner(kind)
    L = pl.lib
    # no columns: H("")
    leaves = DeviceBytes(pl, 4 * 32)
    for variant, want in (("keccak256", bytes.fromhex(KECCAK_EMPTY)), ("sha3_256", hashlib.sha3_256(b"").digest())):
        L.check(L.ms_keccak_rows(pl.handle, VARIANT_ID[variant], FP, 4, None, 0, leaves.ptr))
        assert all(leaves.to_numpy().reshape(4, 32)[r].tobytes() == want for r in range(4))
    # "abc" padded to one 8-byte word is not a row; the published digest of "abc" pins the helper above, a one-element row pins the bytes
    one = Matrix.from_numpy(pl, [cref.to_mont(np.array([1], dtype=np.uint64))])
    assert one.hash_rows("sha3_256").to_numpy().tobytes() == hashlib.sha3_256((1).to_bytes(8, "little")).digest()
    assert one.hash_rows("keccak256").to_numpy().tobytes() == keccak_ref.keccak256((1).to_bytes(8, "little"))
    # a merge of two fixed digests, a fixed proof-of-work nonce
    a, b = hashlib.sha256(b"left").digest(), hashlib.sha256(b"right").digest()
    lv = DeviceBytes(pl, 64)
    L.check(L.ms_upload(pl.handle, lv.ptr, a + b, 64))
    seed = bytes(range(32))
    for variant in VARIANTS:
        assert MerkleTree(pl, lv, 2, variant).root() == h1(variant, a + b)
        assert grind_proof_of_work(pl, seed, 8, hash=variant) == _pow_search(variant, seed, 8)


# ---- 2. rows at every block edge: 17 slots of 8 bytes per block ------------------------------------------------------------------------

NROWS = 257                                                    # one full workgroup and a ragged one


def _want_leaves(variant, field, cols, n):
    return hmany(variant, _row_bytes(field, cols, n))


def _rows_case(kind, variant, field, ncols, seed):
    pl = backends.planner(kind)
    n = NROWS
    cols = [_column(field, n, seed + 17 * c) for c in range(ncols)]
    leaves = DeviceBytes(pl, n * 32)
    vecs = [GpuVec.from_numpy(pl, c, field) for c in cols]
    ptrs = (ctypes.c_void_p * max(1, ncols))(*[v.ptr for v in vecs])
    pl.lib.check(pl.lib.ms_keccak_rows(pl.handle, VARIANT_ID[variant], field, n, ptrs if ncols else None, ncols, leaves.ptr))
    got = leaves.to_numpy().reshape(n, 32)
    want = _want_leaves(variant, field, cols, n) if ncols else [h1(variant, b"")] * n
    for r in range(n):
        assert got[r].tobytes() == want[r], f"row {r}"
    if ncols:                                                  # the name-selected path gives the same leaves
        assert np.array_equal(Matrix(vecs).hash_rows(variant).to_numpy(), leaves.to_numpy())


# Fp: 16 columns put the domain byte and 0x80 in one slot, 17 and 34 are exact multiples of the rate, 128 is the cap;
# Fq3: 6 puts an element across the first block boundary, 17 is three blocks exactly;
# Fp252: 5 and 9 carry the converted element across a boundary, 17 is four blocks exactly
KECCAK_ROWS = ([(FP, c) for c in (0, 1, 8, 16, 17, 18, 33, 34, 35, 128)] + [(FQ3, c) for c in (1, 5, 6, 11, 12, 17, 128)]
               + [(F252, c) for c in (1, 4, 5, 8, 9, 17, 128)])
SHA3_ROWS = [(FP, c) for c in (0, 16, 17, 18)] + [(F252, 5)]
ROW_CASES = [("keccak256", f, c) for f, c in KECCAK_ROWS] + [("sha3_256", f, c) for f, c in SHA3_ROWS]


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("variant,field,ncols", ROW_CASES)
def test_rows_block_edges(kind, variant, field, ncols):
    _rows_case(kind, variant, field, ncols, 101 + ncols)


# ---- 3. row-major FRI layers -------------------------------------------------------------------------------------------------------

def _want_nodes(variant, leaves):
    n = len(leaves)
    nodes = [bytes(32)] * n
    level = list(leaves)
    while len(level) > 1:
        level = hmany(variant, [level[2 * i] + level[2 * i + 1] for i in range(len(level) // 2)])
        nodes[len(level): 2 * len(level)] = level
    return nodes


def _check_tree(variant, tree, leaves):
    got = tree.nodes_numpy()
    want = _want_nodes(variant, leaves)
    assert not got[0].any(), "nodes[0] must stay zero"
    bad = [k for k in range(1, len(leaves)) if got[k].tobytes() != want[k]]
    assert not bad, f"nodes {bad[:8]}"
    assert tree.root() == want[1]


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("field", [FP, FQ3, F252])
@pytest.mark.parametrize("ff", [2, 4, 8, 16])
def test_fri_layer_rows(kind, field, ff):
    pl = backends.planner(kind)
    V = WORDS[field]
    nrows = 255
    ev = _column(field, nrows * ff, 31 + ff)
    vec = GpuVec.from_numpy(pl, ev, field)
    rows = ev.reshape(nrows, ff, V)
    cols = [np.ascontiguousarray(rows[:, k, :]).ravel() for k in range(ff)]           # the de-interleaved layer
    for variant in VARIANTS:
        leaves = DeviceBytes(pl, nrows * 32)
        pl.lib.check(pl.lib.ms_keccak_rows_row_major(pl.handle, VARIANT_ID[variant], field, nrows, ff, vec.ptr, leaves.ptr))
        want = _want_leaves(variant, field, cols, nrows)
        assert [x.tobytes() for x in leaves.to_numpy().reshape(nrows, 32)] == want
        col_major = Matrix.from_numpy(pl, cols, field).hash_rows(variant).to_numpy()
        assert np.array_equal(leaves.to_numpy(), col_major)
    # MerkleTree.from_fri_layer over a power-of-two layer takes the same path
    ev2 = _column(field, 64 * ff, 77 + ff)
    tree = MerkleTree.from_fri_layer(GpuVec.from_numpy(pl, ev2, field), ff, "keccak256")
    rows2 = ev2.reshape(64, ff, V)
    want2 = _want_leaves("keccak256", field, [np.ascontiguousarray(rows2[:, k, :]).ravel() for k in range(ff)], 64)
    assert [x.tobytes() for x in tree.leaves.to_numpy().reshape(64, 32)] == want2
    _check_tree("keccak256", tree, want2)


# ---- 4. trees: every shape of the level / top split -------------------------------------------------------------------------------

def _tree_case(kind, variant, log_n):
    pl = backends.planner(kind)
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    raw = rng.integers(0, 256, size=n * 32, dtype=np.uint8)
    lv = DeviceBytes(pl, n * 32)
    pl.lib.check(pl.lib.ms_upload(pl.handle, lv.ptr, raw.ctypes.data, n * 32))
    tree = MerkleTree(pl, lv, n, variant)
    _check_tree(variant, tree, [raw[32 * i: 32 * i + 32].tobytes() for i in range(n)])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("log_n", list(range(1, 11)) + [12, 17, 18])
def test_tree_shapes_emu(variant, log_n):
    _tree_case("emu", variant, log_n)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("log_n", [1, 5, 9, 10, 13, 17, 18])
def test_tree_shapes_hip(variant, log_n):
    _tree_case("hip", variant, log_n)


# ms_keccak_merkle launches the level kernel only above 2^17 parents, i.e. from 2^19 leaves: 2^19 is one level launch (2^18 parents)
# followed by the PER = 2 subtrees and the top; 2^20 is two level launches, the second reading what the first wrote (src = dst) -- that
# one with SHA3-256 only, whose expected nodes hashlib gives in two seconds (the host's Keccak-256 takes ten; the launches are the same)
LEVEL_CASES = [pytest.param("emu", "keccak256", 19, id="emu-keccak256-19"), pytest.param("emu", "sha3_256", 19, id="emu-sha3_256-19"),
               pytest.param("hip", "keccak256", 19, id="hip-keccak256-19", marks=pytest.mark.gpu),
               pytest.param("hip", "sha3_256", 19, id="hip-sha3_256-19", marks=pytest.mark.gpu),
               pytest.param("hip", "sha3_256", 20, id="hip-sha3_256-20", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("kind,variant,log_n", LEVEL_CASES)
def test_tree_reaches_the_level_kernel(kind, variant, log_n):
    _tree_case(kind, variant, log_n)


# ---- 5. openings ------------------------------------------------------------------------------------------------------------------

def _verify(variant, root, view, indices):
    """MerkleTreeImpl::verify (src/merkle.rs:208-287) with H = Keccak: True iff the batched opening leads to `root`"""
    from collections import deque
    h = lambda d: h1(variant, d)
    n = 1 << view["height"]
    idx = sorted(set(indices))
    siblings, nodes = deque(view["sibling_leaves"]), deque(view["nodes"])
    queue = deque()
    leaves = deque(zip(idx, view["initial_leaves"]))
    while leaves:
        i, leaf = leaves.popleft()
        if leaves and (i ^ 1) == leaves[0][0]:
            queue.append(((n + i) >> 1, h(leaf + leaves.popleft()[1])))
            continue
        s = siblings.popleft()
        queue.append(((n + i) >> 1, h(leaf + s) if i % 2 == 0 else h(s + leaf)))
    while queue:
        i, d = queue.popleft()
        if i == 1:
            return d == root
        if queue and (i ^ 1) == queue[0][0]:
            queue.append((i >> 1, h(d + queue.popleft()[1])))
            continue
        s = nodes.popleft()
        queue.append((i >> 1, h(d + s) if i % 2 == 0 else h(s + d)))
    return False


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", BACKENDS)
def test_openings_verify_against_the_root(kind, variant):
    pl = backends.planner(kind)
    n = 256
    cols = [_column(FP, n, 77 + 17 * c) for c in range(9)]
    m = Matrix.from_numpy(pl, cols, FP)
    want = _want_leaves(variant, FP, cols, n)
    tree = MerkleTree.from_matrix(m, variant)
    root = tree.root()
    for indices in ([0], [255], [3, 4, 5, 200], [1, 17, 18, 19, 100, 101, 254]):
        view = tree.prove(indices)
        assert view["initial_leaves"] == [want[i] for i in sorted(set(indices))]
        assert _verify(variant, root, view, indices)
        bad = dict(view, initial_leaves=list(view["initial_leaves"]))
        leaf = bytearray(bad["initial_leaves"][0])
        leaf[5] ^= 0x10
        bad["initial_leaves"][0] = bytes(leaf)
        assert not _verify(variant, root, bad, indices)


# ---- 6. proof of work ------------------------------------------------------------------------------------------------------------

def _pow_search(variant, seed, bits):
    n = 1
    while True:                                                # in batches: the expected nonce is about 2^bits
        digests = hmany(variant, [seed + k.to_bytes(8, "big") for k in range(n, n + 512)])
        for k, d in enumerate(digests):
            if _lz(d) >= bits:
                return n + k
        n += 512


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", BACKENDS)
def test_pow_matches_linear_search(kind, variant):
    pl = backends.planner(kind)
    seed = hashlib.sha256(bytes([3, 7])).digest()
    answers = {}
    for bits in (0, 1, 9, 12):
        answers[bits] = _pow_search(variant, seed, bits)
        assert grind_proof_of_work(pl, seed, bits, 1 << 32, hash=variant) == answers[bits], bits
    assert answers[0] == 1
    need = answers[9]
    assert grind_proof_of_work(pl, seed, 9, need, hash=variant) == need          # max_nonce exactly at the answer
    with pytest.raises(MsError, match="no nonce below") as e:
        grind_proof_of_work(pl, seed, 9, need - 1, hash=variant)                  # and one below it
    assert e.value.code == -1
    with pytest.raises(MsError, match="bits must be <= 64") as e:
        grind_proof_of_work(pl, seed, 65, hash=variant)
    assert e.value.code == -1


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------

def test_error_paths_emu():
    pl = backends.planner("emu")
    L = pl.lib
    K = 0
    col = GpuVec.from_numpy(pl, cref.random_elements(8, 1))
    cols = (ctypes.c_void_p * 1)(col.ptr)
    out = DeviceBytes(pl, 8 * 32)
    out2 = DeviceBytes(pl, 8 * 32)
    before = out.to_numpy().copy()
    seed = ctypes.create_string_buffer(32)
    nonce = ctypes.c_uint64(0)
    for rc in (L.ms_keccak_rows(None, K, FP, 8, cols, 1, out.ptr), L.ms_keccak_rows(pl.handle, K, FP, 8, None, 1, out.ptr),
               L.ms_keccak_rows(pl.handle, K, FP, 8, cols, 1, None), L.ms_keccak_rows(pl.handle, K, FP, 8, (ctypes.c_void_p * 1)(None), 1, out.ptr),
               L.ms_keccak_rows_row_major(pl.handle, K, FP, 8, 1, None, out.ptr), L.ms_keccak_rows_row_major(None, K, FP, 8, 1, col.ptr, out.ptr),
               L.ms_keccak_merkle(pl.handle, K, 8, None, out2.ptr), L.ms_keccak_merkle(pl.handle, K, 8, out.ptr, None),
               L.ms_keccak_pow_grind(pl.handle, K, None, 1, 10, ctypes.byref(nonce)), L.ms_keccak_pow_grind(pl.handle, K, seed, 1, 10, None),
               # unknown variant 2 (and a negative one), on every entry point
               L.ms_keccak_rows(pl.handle, 2, FP, 8, cols, 1, out.ptr), L.ms_keccak_rows_row_major(pl.handle, 2, FP, 8, 1, col.ptr, out.ptr),
               L.ms_keccak_merkle(pl.handle, 2, 8, out.ptr, out2.ptr), L.ms_keccak_pow_grind(pl.handle, 2, seed, 1, 10, ctypes.byref(nonce)),
               L.ms_keccak_rows(pl.handle, -1, FP, 8, cols, 1, out.ptr)):
        assert rc == -1
    with pytest.raises(MsError, match="unknown variant 2"):
        L.check(L.ms_keccak_merkle(pl.handle, 2, 8, out.ptr, out2.ptr))
    many = (ctypes.c_void_p * 129)(*([col.ptr] * 129))
    with pytest.raises(MsError, match="at most 128 columns") as e:
        L.check(L.ms_keccak_rows(pl.handle, K, FP, 8, many, 129, out.ptr))
    assert e.value.code == -2
    for ncols in (0, 129):
        with pytest.raises(MsError, match="1..128 columns") as e:
            L.check(L.ms_keccak_rows_row_major(pl.handle, K, FP, 1, ncols, col.ptr, out.ptr))
        assert e.value.code == -2
    with pytest.raises(MsError, match="power of two"):
        L.check(L.ms_keccak_merkle(pl.handle, K, 3, out.ptr, out2.ptr))
    with pytest.raises(MsError, match="power of two"):
        L.check(L.ms_keccak_merkle(pl.handle, K, 1, out.ptr, out2.ptr))
    with pytest.raises(MsError, match="unknown field id 7"):
        L.check(L.ms_keccak_rows(pl.handle, K, 7, 8, cols, 1, out.ptr))
    with pytest.raises(MsError, match="unknown field id 9"):
        L.check(L.ms_keccak_rows_row_major(pl.handle, K, 9, 8, 1, col.ptr, out.ptr))
    assert np.array_equal(out.to_numpy(), before)              # every refusal came before anything was enqueued
    # the names: the new ones are accepted, the old unknown ones still refused
    m = Matrix([col])
    for variant in VARIANTS:
        assert MerkleTree.from_matrix(m, variant).hash == variant
        assert grind_proof_of_work(pl, bytes(32), 0, hash=variant) == 1
    with pytest.raises(ValueError, match="unknown hash"):
        m.hash_rows("blake3")
    with pytest.raises(ValueError, match="unknown hash"):
        MerkleTree(pl, out, 8, "keccak")
    with pytest.raises(ValueError, match="unknown proof-of-work hash"):
        grind_proof_of_work(pl, bytes(32), 1, hash="rpo256")


# ---- 8. checked mode ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", BACKENDS)
def test_checked_mode_refuses_non_canonical_rows(kind):
    pl = backends.planner(kind)
    L = pl.lib
    n = 16
    GL_P, P252 = cref.GL_P, cref.F252_P
    cases = []
    fp = [_column(FP, n, 5 + c) for c in range(3)]
    fp[1][9] = GL_P + 3                                        # an Fp column: column 1, row 9
    cases.append((FP, fp, r"column 1, row 9"))
    q3 = [_column(FQ3, n, 9 + c) for c in range(2)]
    q3[1][3 * 4 + 2] = (1 << 64) - 1                           # an Fq3 component: column 1, row 4, component 2
    cases.append((FQ3, q3, r"column 1, row 4, component 2"))
    big = [_column(F252, n, 13 + c) for c in range(2)]
    big[0][4 * 7: 4 * 7 + 4] = [(P252 >> (64 * k)) & ((1 << 64) - 1) for k in range(4)]   # an Fp252 element equal to p: column 0, row 7
    cases.append((F252, big, r"column 0, row 7"))
    for field, cols, where in cases:
        vecs = [GpuVec.from_numpy(pl, c, field) for c in cols]
        ptrs = (ctypes.c_void_p * len(vecs))(*[v.ptr for v in vecs])
        leaves = DeviceBytes(pl, n * 32)
        L.check(L.ms_upload(pl.handle, leaves.ptr, bytes([0xA5]) * (n * 32), n * 32))
        pl.checked(True)
        try:
            for variant in (0, 1):
                with pytest.raises(MsError, match=r"ms_keccak_rows: d_cols holds an element that is not canonical.*" + where) as e:
                    L.check(L.ms_keccak_rows(pl.handle, variant, field, n, ptrs, len(vecs), leaves.ptr))
                assert e.value.code == -1
                assert set(leaves.to_numpy().tolist()) == {0xA5}, "the leaves buffer must be untouched"
        finally:
            pl.checked(False)
        L.check(L.ms_keccak_rows(pl.handle, 0, field, n, ptrs, len(vecs), leaves.ptr))          # checked mode off: not refused
        assert set(leaves.to_numpy().tolist()) != {0xA5}
    # the row-major form scans too
    bad = _column(FP, n * 4, 3)
    bad[4 * 5 + 2] = GL_P
    vec = GpuVec.from_numpy(pl, bad, FP)
    leaves = DeviceBytes(pl, n * 32)
    pl.checked(True)
    try:
        with pytest.raises(MsError, match=r"ms_keccak_rows_row_major: d_matrix holds an element that is not canonical"):
            L.check(L.ms_keccak_rows_row_major(pl.handle, 0, FP, n, 4, vec.ptr, leaves.ptr))
    finally:
        pl.checked(False)
    L.check(L.ms_keccak_rows_row_major(pl.handle, 0, FP, n, 4, vec.ptr, leaves.ptr))
