"""Sweep of the RPO-256 commitment entry points through the C ABI: ms_rpo256_rows, ms_rpo256_rows_row_major, ms_rpo256_rows_field and
ms_rpo256_merkle (kernels rpo256_rows, rpo256_merge_level_wide and rpo256_merge_level of csrc/rpo_kernels.h).  Row counts around a
workgroup's 256 lanes, column counts around the absorb edges (8 words per absorb) and at the limit of 128, the row-major stride, Fq3 rows,
edge-valued rows and the padding rule, every refusal, every node of small trees, and every output of the one-lane merge kernel.

All comparisons are word for word.  The reference is oracle/pyref/rpo.py (Python integers, pinned to external vectors by
tests/test_rpo_parity.py); it costs 1.6 ms per permutation, so a table with many rows gives row r the data of row r mod PERIOD: the
first PERIOD digests are compared with the oracle and every other digest with the digest of its class, which checks every output word.
Every digest buffer is one digest longer than the call needs, filled with a sentinel, and carries guard words behind it."""
import ctypes
import functools

import numpy as np
import pytest

from oracle.pyref import rpo as pyrpo
from oracle.pyref.fields import GL
from tests import backends
from tests.test_stage_sweep import Buf, gl_values, same
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as F252

P = GL.p
MS_OK, MS_ERR_INVALID, MS_ERR_UNSUPPORTED = 0, -1, -2
KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
JUNK = 0xDEADBEEFDEADBEEF
MAXCOLS = 128
PERIOD = 4
VP = ctypes.c_void_p
ONE = GL.to_mont(1)


# ------------------------------------------------------------------------------------------------------------------
# the reference, on Montgomery words
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _digest(row):
    return tuple(GL.to_mont(x) for x in pyrpo.hash_row([GL.from_mont(w) for w in row]))


def digest(row):
    """the four words of the oracle's digest of a row of canonical Montgomery words (kept: the emu and hip runs share their tables)"""
    return _digest(tuple(int(w) for w in row))


def table(nrows, nwords, seed, period=PERIOD):
    """nrows x nwords canonical words, row r = row r mod period; uniform words with the carry-edge words sprinkled in"""
    base = gl_values(period * nwords, 1, seed).reshape(period, nwords)
    return np.ascontiguousarray(base[np.arange(nrows) % period])


def period_for(nrows, nwords):
    """every row its own where the oracle can afford it (one absorb per row, up to 257 rows)"""
    return max(nrows, 1) if nrows * ((nwords + 7) // 8) <= 257 else PERIOD


class Digests:
    """nrows digests and one more, all sentinel words before the call"""

    def __init__(self, pl, nrows):
        self.nrows, self.buf = nrows, Buf.junk(pl, 4 * (nrows + 1))
        self.ptr = self.buf.ptr

    def read(self, what):
        got = self.buf.read()
        same(got[4 * self.nrows:], np.full(4, JUNK, dtype=np.uint64), what + ": the digest behind the last row")
        return got[:4 * self.nrows].reshape(self.nrows, 4)

    def untouched(self, what):
        same(self.buf.read(), np.full(4 * (self.nrows + 1), JUNK, dtype=np.uint64), what)


def check(got, rows, period, what):
    """the first `period` digests against the oracle, every digest against the digest of its class"""
    nrows = rows.shape[0]
    k = min(period, nrows)
    want = np.array([digest(rows[r]) for r in range(k)], dtype=np.uint64).reshape(k, 4)
    same(got[:k].reshape(-1), want.reshape(-1), what + ": the first rows against the oracle")
    same(got.reshape(-1), got[np.arange(nrows) % period].reshape(-1), what + ": every row against the row of its class")


def column_major(pl, rows, what):
    nrows, ncols = rows.shape
    cols = [Buf(pl, np.ascontiguousarray(rows[:, c])) for c in range(ncols)]
    out = Digests(pl, nrows)
    rc = pl.lib.ms_rpo256_rows(pl.handle, nrows, (VP * ncols)(*[c.ptr for c in cols]), ncols, out.ptr)
    assert rc == MS_OK, pl.lib.ms_last_error()
    got = out.read(what)
    for c, col in enumerate(cols):
        same(col.read(), rows[:, c], f"{what}: column {c} after the call")
    return got


def row_major(pl, rows, what):
    nrows, ncols = rows.shape
    M, out = Buf(pl, rows.reshape(-1)), Digests(pl, nrows)
    rc = pl.lib.ms_rpo256_rows_row_major(pl.handle, nrows, ncols, M.ptr, out.ptr)
    assert rc == MS_OK, pl.lib.ms_last_error()
    got = out.read(what)
    same(M.read(), rows.reshape(-1), what + ": the matrix after the call")
    return got


def by_field(pl, field, rows, what):
    """rows: nrows x (ncols V) words; column c holds the V words of its element of row r at [r V, (r + 1) V)"""
    v = 3 if field == FQ3 else 1
    nrows, ncols = rows.shape[0], rows.shape[1] // v
    cols = [Buf(pl, np.ascontiguousarray(rows[:, v * c:v * c + v]).reshape(-1)) for c in range(ncols)]
    out = Digests(pl, nrows)
    rc = pl.lib.ms_rpo256_rows_field(pl.handle, field, nrows, (VP * ncols)(*[c.ptr for c in cols]), ncols, out.ptr)
    assert rc == MS_OK, pl.lib.ms_last_error()
    return out.read(what)


# ------------------------------------------------------------------------------------------------------------------
# rpo256_rows: row counts at the workgroup edge (NT = 256), column counts at the absorb edges and at the limit
# ------------------------------------------------------------------------------------------------------------------
ROW_COUNTS = (1, 2, 255, 256, 257, 513)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ncols", [1, 8, 9])
def test_row_counts_at_the_workgroup_edge(kind, ncols):
    """the last lane of a workgroup, the first lane of the next, a partly filled last workgroup; nothing behind the last digest"""
    pl = backends.planner(kind)
    for nrows in ROW_COUNTS:
        period = period_for(nrows, ncols)
        rows = table(nrows, ncols, 1000 * ncols + nrows, period)
        what = f"ms_rpo256_rows {nrows} rows of {ncols} columns"
        check(column_major(pl, rows, what), rows, period, what)


COLUMN_COUNTS = (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 127, 128)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ncols", COLUMN_COUNTS)
def test_column_counts_at_the_absorb_edges(kind, ncols):
    """one word short of a full absorb, a full one, one word into the next, for one to four absorbs and at the limit of sixteen; the
    row-major call runs at stride ncols; the three entry points agree on the same data"""
    pl = backends.planner(kind)
    nrows = 257
    period = period_for(nrows, ncols)                           # up to 8 columns: every row its own
    rows = table(nrows, ncols, 77 + ncols, period)
    a = column_major(pl, rows, f"ms_rpo256_rows {ncols} columns")
    check(a, rows, period, f"ms_rpo256_rows {ncols} columns")
    b = row_major(pl, rows, f"ms_rpo256_rows_row_major {ncols} columns")
    check(b, rows, period, f"ms_rpo256_rows_row_major {ncols} columns")
    c = by_field(pl, FP, rows, f"ms_rpo256_rows_field Fp {ncols} columns")
    check(c, rows, period, f"ms_rpo256_rows_field Fp {ncols} columns")
    same(b.reshape(-1), a.reshape(-1), "row-major against column-major")
    same(c.reshape(-1), a.reshape(-1), "ms_rpo256_rows_field against ms_rpo256_rows")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ncols", [1, 2, 3, 5, 8, 42])
def test_fq3_rows(kind, ncols):
    """an Fq3 column contributes c0, c1, c2 in this order (42 columns: 126 absorbed words); the same digests from the Fp call on the
    3 ncols component columns"""
    pl = backends.planner(kind)
    nrows = 257
    rows = table(nrows, 3 * ncols, 300 + ncols)
    a = by_field(pl, FQ3, rows, f"ms_rpo256_rows_field Fq3 {ncols} columns")
    check(a, rows, PERIOD, f"ms_rpo256_rows_field Fq3 {ncols} columns")
    b = by_field(pl, FP, rows, f"ms_rpo256_rows_field Fp {3 * ncols} component columns")
    same(b.reshape(-1), a.reshape(-1), "Fp on the component columns against Fq3")


@pytest.mark.parametrize("kind", KINDS)
def test_edge_valued_rows(kind):
    """all zero, all p - 1 (as a word and as a value), a single 1 (as a value and as a word) followed by zeros: every row its own"""
    pl = backends.planner(kind)
    for ncols in (1, 7, 8, 9, 15, 16, 17, MAXCOLS):
        rows = np.zeros((5, ncols), dtype=np.uint64)
        rows[1, :] = P - 1
        rows[2, :] = GL.to_mont(P - 1)
        rows[3, 0] = ONE
        rows[4, 0] = 1
        for call in (column_major, row_major):
            check(call(pl, rows, f"{call.__name__} edge rows of {ncols} columns"), rows, 5, f"{call.__name__} edge rows of {ncols} columns")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("short", [7, 15])
def test_padding_separates_a_row_from_its_padded_form(kind, short):
    """a row of 7 (15) elements is absorbed as the row with a 1 appended -- the same rate words as the 8 (16)-element row that ends in
    1 -- and differs from it only in the capacity word: the digests must differ, and each must be the oracle's"""
    pl = backends.planner(kind)
    x = table(3, short, 500 + short, 3)
    x[2, :] = 0                                                  # ... and the all-zero row against (0, .., 0, 1)
    y = np.concatenate([x, np.full((3, 1), ONE, dtype=np.uint64)], axis=1)
    a = column_major(pl, x, f"{short} columns")
    b = column_major(pl, y, f"{short + 1} columns")
    check(a, x, 3, f"{short} columns")
    check(b, y, 3, f"{short + 1} columns")
    for r in range(3):
        assert digest(x[r]) != digest(y[r])
        assert not np.array_equal(a[r], b[r]), f"row {r}: the {short}-element row and its padded form have one digest"


# ------------------------------------------------------------------------------------------------------------------
# refusals: the return code, the text of ms_last_error, and nothing written
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    pl = backends.planner(kind)
    L, h = pl.lib, pl.handle
    nrows = 4
    src = table(nrows, 129, 9)
    S = Buf(pl, src.reshape(-1))                                 # 129 columns of 4 rows, or a row-major matrix, or 43 Fq3 columns
    out = Digests(pl, nrows)
    cols = (VP * 129)(*[S.ptr + 8 * nrows * c for c in range(129)])
    q3 = (VP * 43)(*[S.ptr + 8 * 3 * nrows * c for c in range(43)])

    def refused(rc, code, text):
        msg = L.ms_last_error().decode()
        assert rc == code and text in msg, (rc, msg)

    refused(L.ms_rpo256_rows(h, nrows, cols, 0, out.ptr), MS_ERR_INVALID, "zero-length input")
    refused(L.ms_rpo256_rows_field(h, FP, nrows, cols, 0, out.ptr), MS_ERR_INVALID, "zero-length input")
    refused(L.ms_rpo256_rows_field(h, FQ3, nrows, cols, 0, out.ptr), MS_ERR_INVALID, "zero-length input")
    refused(L.ms_rpo256_rows_row_major(h, nrows, 0, S.ptr, out.ptr), MS_ERR_INVALID, "zero-length input")
    refused(L.ms_rpo256_rows(h, nrows, cols, MAXCOLS + 1, out.ptr), MS_ERR_UNSUPPORTED, "at most 128 columns")
    refused(L.ms_rpo256_rows_field(h, FP, nrows, cols, MAXCOLS + 1, out.ptr), MS_ERR_UNSUPPORTED, "at most 128 columns")
    refused(L.ms_rpo256_rows_row_major(h, nrows, MAXCOLS + 1, S.ptr, out.ptr), MS_ERR_UNSUPPORTED, "at most 128 columns")
    refused(L.ms_rpo256_rows_field(h, FQ3, nrows, q3, 43, out.ptr), MS_ERR_UNSUPPORTED, "at most 128 columns")        # 129 words
    refused(L.ms_rpo256_rows_field(h, F252, nrows, cols, 2, out.ptr), MS_ERR_UNSUPPORTED, "Goldilocks")
    for ncols in (1, 9, MAXCOLS):                                # no rows: nothing to do
        assert L.ms_rpo256_rows(h, 0, cols, ncols, out.ptr) == MS_OK
        assert L.ms_rpo256_rows_field(h, FP, 0, cols, ncols, out.ptr) == MS_OK
        assert L.ms_rpo256_rows_row_major(h, 0, ncols, S.ptr, out.ptr) == MS_OK
    assert L.ms_rpo256_rows_field(h, FQ3, 0, q3, 42, out.ptr) == MS_OK
    # null arguments
    refused(L.ms_rpo256_rows(None, nrows, cols, 2, out.ptr), MS_ERR_INVALID, "ms_rpo256_rows: null argument")
    refused(L.ms_rpo256_rows(h, nrows, None, 2, out.ptr), MS_ERR_INVALID, "ms_rpo256_rows: null argument")
    refused(L.ms_rpo256_rows(h, nrows, cols, 2, None), MS_ERR_INVALID, "ms_rpo256_rows: null argument")
    refused(L.ms_rpo256_rows_field(None, FP, nrows, cols, 2, out.ptr), MS_ERR_INVALID, "ms_rpo256_rows_field: null argument")
    refused(L.ms_rpo256_rows_field(h, FP, nrows, None, 2, out.ptr), MS_ERR_INVALID, "ms_rpo256_rows_field: null argument")
    refused(L.ms_rpo256_rows_field(h, FQ3, nrows, cols, 2, None), MS_ERR_INVALID, "ms_rpo256_rows_field: null argument")
    refused(L.ms_rpo256_rows_row_major(None, nrows, 2, S.ptr, out.ptr), MS_ERR_INVALID, "ms_rpo256_rows_row_major: null argument")
    refused(L.ms_rpo256_rows_row_major(h, nrows, 2, None, out.ptr), MS_ERR_INVALID, "ms_rpo256_rows_row_major: null argument")
    refused(L.ms_rpo256_rows_row_major(h, nrows, 2, S.ptr, None), MS_ERR_INVALID, "ms_rpo256_rows_row_major: null argument")
    # a null column among the columns: both column-major entry points name it
    for ncols, at in ((1, 0), (3, 0), (3, 1), (9, 8), (MAXCOLS, MAXCOLS - 1)):
        holed = (VP * 129)(*[None if c == at else S.ptr + 8 * nrows * c for c in range(129)])
        refused(L.ms_rpo256_rows(h, nrows, holed, ncols, out.ptr), MS_ERR_INVALID, f"null column {at}")
        refused(L.ms_rpo256_rows_field(h, FP, nrows, holed, ncols, out.ptr), MS_ERR_INVALID, f"null column {at}")
    pl.sync()
    out.untouched("the digests after the refused calls")
    same(S.read(), src.reshape(-1), "the source after the refused calls")


@pytest.mark.parametrize("kind", KINDS)
def test_merkle_refusals(kind):
    pl = backends.planner(kind)
    L, h = pl.lib, pl.handle
    src = table(8, 4, 10, 8)
    leaves, nodes = Buf(pl, src.reshape(-1)), Buf.junk(pl, 4 * 8)
    for nleaves in (0, 1, 3, 6):
        assert L.ms_rpo256_merkle(h, nleaves, leaves.ptr, nodes.ptr) == MS_ERR_INVALID
        assert b"power of two" in L.ms_last_error()
    for args in ((None, 8, leaves.ptr, nodes.ptr), (h, 8, None, nodes.ptr), (h, 8, leaves.ptr, None)):
        assert L.ms_rpo256_merkle(*args) == MS_ERR_INVALID
        assert b"ms_rpo256_merkle: null argument" in L.ms_last_error()
    pl.sync()
    same(nodes.read(), np.full(32, JUNK, dtype=np.uint64), "the nodes after the refused calls")
    same(leaves.read(), src.reshape(-1), "the leaves after the refused calls")


# ------------------------------------------------------------------------------------------------------------------
# trees
# ------------------------------------------------------------------------------------------------------------------
def merkle(pl, leaf_words):
    """-> the nleaves x 4 node words; the node buffer is all sentinel before the call, the leaves are compared after it"""
    nleaves = leaf_words.size // 4
    leaves, nodes = Buf(pl, leaf_words), Buf.junk(pl, 4 * nleaves)
    rc = pl.lib.ms_rpo256_merkle(pl.handle, nleaves, leaves.ptr, nodes.ptr)
    assert rc == MS_OK, pl.lib.ms_last_error()
    got = nodes.read().reshape(nleaves, 4)
    same(leaves.read(), leaf_words, f"the {nleaves} leaves after the call")
    return got


@functools.lru_cache(maxsize=None)
def tree(nleaves):
    """(leaf words, the oracle's node words): nleaves - 1 permutations, once for both backends"""
    words = gl_values(4 * nleaves, 1, 600 + nleaves)
    vals = [[GL.from_mont(int(w)) for w in words[4 * i:4 * i + 4]] for i in range(nleaves)]
    want = np.array([[GL.to_mont(x) for x in d] for d in pyrpo.merkle_nodes(vals)], dtype=np.uint64)
    return words, want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nleaves", [2, 4, 8, 16, 512, 1024])
def test_tree_every_node(kind, nleaves):
    """rpo256_merge_level_wide holds four nodes per workgroup: the levels of 1 and 2 nodes are a partly live workgroup, the level of 4 the
    first full one, the level of 512 has 128 workgroups.  nodes[0] is zero, nodes[1] the root."""
    pl = backends.planner(kind)
    words, want = tree(nleaves)
    got = merkle(pl, words)
    same(got[0], np.zeros(4, dtype=np.uint64), "nodes[0]")
    same(got[1:].reshape(-1), want[1:].reshape(-1), f"the nodes of {nleaves} leaves against the oracle")


@pytest.mark.gpu
def test_one_lane_merge_kernel_every_output():
    """ms_rpo256_merkle runs a level of more than 2^15 nodes on rpo256_merge_level (one lane per node) and every other level on
    rpo256_merge_level_wide.  At 2^17 leaves the level of 2^16 nodes is the only one of the first kind.  The same leaves cut into four
    quarters of 2^15 give four trees whose first level has 2^14 nodes, computed by the wide kernel, which test_tree_every_node pins to the
    oracle: concatenated, the four first levels must be nodes[2^16, 2^17) of the big tree, all 65 536 digests.  (Both kernels report
    to the profile as rpo256_merkle_level, one call per level: the kernel is told by the level's size.)  A sample of that level is
    compared with the oracle directly."""
    pl = backends.planner("hip")
    n, q = 1 << 17, 1 << 15
    words = gl_values(4 * n, 1, 4242)
    pl.profile(True)
    big = merkle(pl, words)
    prof = pl.profile_read()
    pl.profile(False)
    assert prof["rpo256_merkle_level"]["calls"] == 17, prof
    level = big[n // 2:n]
    quarters = []
    for k in range(4):
        pl.profile(True)
        sub = merkle(pl, words[4 * q * k:4 * q * (k + 1)])
        prof = pl.profile_read()
        pl.profile(False)
        assert prof["rpo256_merkle_level"]["calls"] == 15, prof
        quarters.append(sub[q // 2:q])
    same(np.concatenate(quarters).reshape(-1), level.reshape(-1), "the level of 2^16 nodes: one lane per node against sixteen lanes per node")
    lv = words.reshape(n, 4)
    for i in [0, 1, 255, 256, 257, n // 2 - 1] + [int(x) for x in np.random.default_rng(8).integers(0, n // 2, size=6)]:
        want = pyrpo.merge([GL.from_mont(int(w)) for w in lv[2 * i]], [GL.from_mont(int(w)) for w in lv[2 * i + 1]])
        assert [GL.from_mont(int(w)) for w in level[i]] == want, i
