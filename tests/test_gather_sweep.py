"""Sweep of the movers through the C ABI: ms_deinterleave (kernel deinterleave), ms_gather_rows (gather_rows), ms_gather_digests (gather_records)
and ms_gather_digests_multi (copy_records32), all in csrc/scan_kernels.h.  They move 64-bit words and compute nothing, so the reference is numpy
indexing.  Shapes: the three element widths (Fp 1 word, Fq3 3, Fp252 4), 1 / 2 / 3 / 7 / 128 columns, row counts around a workgroup's 256 lanes,
position lists with 0, the last row, repeats and a descending run -- and for every kernel one shape past stream_grid's cap of 4096 workgroups x
256 lanes = 2^20 words, where a lane takes a second word.

Every output lies in an arena of sentinel words with at least 16 of them behind every column, and the whole arena is compared; the sources are
compared after the call.  The second half checks the aliasing rule of include/ministark_hip.h: an output over a source, or over another output,
is refused with MS_ERR_INVALID and "overlap" before anything is enqueued, and the arena is left as it was."""
import ctypes

import numpy as np
import pytest

from tests import backends
from tests.test_stage_sweep import M252, Buf, same
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as F252

V = {FP: 1, FQ3: 3, F252: 4}
FNAME = {FP: "fp", FQ3: "fq3", F252: "f252"}
FIELDS = (FP, FQ3, F252)
FIELD_IDS = [FNAME[f] for f in FIELDS]
MS_OK, MS_ERR_INVALID, MS_ERR_UNSUPPORTED = 0, -1, -2
KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
CAP = 1 << 20                       # stream_grid: 4096 workgroups of 256 lanes
MAXCOLS = 128
JUNK = 0xDEADBEEFDEADBEEF
GAP = 16                            # sentinel words behind every output column
VP, SZ = ctypes.c_void_p, ctypes.c_size_t


def words(field, n, seed):
    """n elements: any words will do for a mover; for the 252-bit field they are canonical Montgomery words all the same"""
    if field == F252:
        return M252.values(n, seed)
    return np.random.default_rng(seed).integers(0, 1 << 64, size=n * V[field], dtype=np.uint64)


class Arena:
    """`count` output columns of `colwords` words each, GAP sentinel words behind every one, in one device buffer"""

    def __init__(self, pl, count, colwords):
        self.count, self.colwords, self.stride = count, colwords, colwords + GAP
        self.buf = Buf.junk(pl, count * self.stride)
        self.ptrs = [self.buf.ptr + 8 * c * self.stride for c in range(count)]

    def check(self, columns, what):
        want = np.full((self.count, self.stride), JUNK, dtype=np.uint64)
        for c, col in enumerate(columns):
            want[c, :self.colwords] = col
        same(self.buf.read(), want.reshape(-1), what)


# ------------------------------------------------------------------------------------------------------------------
# ms_deinterleave: d_out[c][j] = d_in[j k + c]
# ------------------------------------------------------------------------------------------------------------------
def run_deinterleave(pl, field, n_out, k, seed):
    v = V[field]
    src = words(field, n_out * k, seed)
    S, out = Buf(pl, src), Arena(pl, k, n_out * v)
    rc = pl.lib.ms_deinterleave(pl.handle, field, n_out, k, S.ptr, (VP * k)(*out.ptrs))
    assert rc == MS_OK, pl.lib.ms_last_error()
    cube = src.reshape(n_out, k, v)
    out.check([cube[:, c, :].reshape(-1) for c in range(k)], f"deinterleave {FNAME[field]} n_out {n_out} k {k}")
    same(S.read(), src, "d_in")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [1, 2, 3, 7, MAXCOLS])
@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_deinterleave(kind, field, k):
    pl = backends.planner(kind)
    for n_out in (1, 2, 255, 257):
        run_deinterleave(pl, field, n_out, k, 10 * k + n_out)


DEINTERLEAVE_LONG = (FQ3, 49933, 7)          # 49933 * 7 * 3 = 2^20 + 17 words: the last 17 are second words of the first 17 lanes


@pytest.mark.parametrize("kind", KINDS)
def test_deinterleave_past_the_grid_cap(kind):
    field, n_out, k = DEINTERLEAVE_LONG
    assert n_out * k * V[field] > CAP + 3
    run_deinterleave(backends.planner(kind), field, n_out, k, 5)


@pytest.mark.parametrize("kind", KINDS)
def test_deinterleave_refuses_0_and_129_columns(kind):
    pl = backends.planner(kind)
    src = words(FP, 4 * 129, 1)
    S, out = Buf(pl, src), Arena(pl, 129, 4)
    for field in FIELDS:
        for k in (0, MAXCOLS + 1):
            assert pl.lib.ms_deinterleave(pl.handle, field, 1, k, S.ptr, (VP * 129)(*out.ptrs)) == MS_ERR_UNSUPPORTED
    assert pl.lib.ms_deinterleave(pl.handle, FP, 0, 3, S.ptr, (VP * 129)(*out.ptrs)) == MS_OK              # no rows: nothing to do
    pl.sync()
    out.check([], "the outputs of refused calls")
    same(S.read(), src, "d_in")


# ------------------------------------------------------------------------------------------------------------------
# ms_gather_rows: out[p][c] = cols[c][positions[p]]
# ------------------------------------------------------------------------------------------------------------------
def positions_for(nrows, npos, seed):
    """0, the last row, repeats, a descending run; uniform draws up to npos"""
    head = [0, nrows - 1, nrows - 1, 0, 5 % nrows, 5 % nrows, 5 % nrows] + list(range(nrows - 1, max(nrows - 40, -1), -1))
    rest = np.random.default_rng(seed).integers(0, nrows, size=max(0, npos - len(head))).tolist()
    return np.array((head + rest)[:npos], dtype=np.uint64)


def run_gather_rows(pl, field, nrows, ncols, npos, seed):
    v = V[field]
    src = words(field, ncols * nrows, seed)                                    # the columns one after another (they are only read)
    pos = positions_for(nrows, npos, seed + 1)
    S, out = Buf(pl, src), Arena(pl, 1, npos * ncols * v)
    cols = (VP * ncols)(*[S.ptr + 8 * c * nrows * v for c in range(ncols)])
    rc = pl.lib.ms_gather_rows(pl.handle, field, nrows, cols, ncols, pos.ctypes.data, npos, out.ptrs[0])
    assert rc == MS_OK, pl.lib.ms_last_error()
    want = src.reshape(ncols, nrows, v)[:, pos.astype(np.int64), :].transpose(1, 0, 2)      # [position][column][word]
    out.check([want.reshape(-1)], f"gather_rows {FNAME[field]} {ncols} columns of {nrows} rows, {npos} positions")
    same(S.read(), src, "the columns")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ncols", [1, 2, MAXCOLS])
@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_gather_rows(kind, field, ncols):
    pl = backends.planner(kind)
    for nrows, npos in ((1, 3), (64, 1), (64, 90), (257, 300)):
        run_gather_rows(pl, field, nrows, ncols, npos, 100 * ncols + nrows)


@pytest.mark.parametrize("kind", KINDS)
def test_gather_rows_past_the_grid_cap(kind):
    nrows, ncols, npos = 64, MAXCOLS, 2800                                     # 2800 * 128 * 3 = 2^20 + 26 624 words
    assert npos * ncols * V[FQ3] > CAP
    run_gather_rows(backends.planner(kind), FQ3, nrows, ncols, npos, 7)


@pytest.mark.parametrize("kind", KINDS)
def test_gather_rows_refuses_129_columns_and_a_row_past_the_end(kind):
    pl = backends.planner(kind)
    L, nrows = pl.lib, 64
    for field in FIELDS:
        v = V[field]
        src = words(field, 2 * nrows, 3)
        S, out = Buf(pl, src), Arena(pl, 1, 8 * 129 * v)
        cols = (VP * 129)(*([S.ptr, S.ptr + 8 * nrows * v] * 64 + [S.ptr]))
        pos = np.array([0, 5, nrows - 1, 7], dtype=np.uint64)
        assert L.ms_gather_rows(pl.handle, field, nrows, cols, MAXCOLS + 1, pos.ctypes.data, 4, out.ptrs[0]) == MS_ERR_UNSUPPORTED
        assert L.ms_gather_rows(pl.handle, field, nrows, cols, 0, pos.ctypes.data, 4, out.ptrs[0]) == MS_ERR_UNSUPPORTED
        pos[2] = nrows
        assert L.ms_gather_rows(pl.handle, field, nrows, cols, 2, pos.ctypes.data, 4, out.ptrs[0]) == MS_ERR_INVALID
        assert b"out of range" in L.ms_last_error()
        pl.sync()
        out.check([], "the output of refused calls")
        same(S.read(), src, "the columns")


# ------------------------------------------------------------------------------------------------------------------
# ms_gather_digests, ms_gather_digests_multi: 32-byte records
# ------------------------------------------------------------------------------------------------------------------
def gather_single(pl, src, idx, what):
    S, out = Buf(pl, src), Arena(pl, 1, 4 * len(idx))
    rc = pl.lib.ms_gather_digests(pl.handle, src.size // 4, S.ptr, idx.ctypes.data, len(idx), out.ptrs[0])
    assert rc == MS_OK, pl.lib.ms_last_error()
    out.check([src.reshape(-1, 4)[idx.astype(np.int64)].reshape(-1)], what)
    same(S.read(), src, what + ": the digests")


def gather_multi(pl, srcs, idxs, what):
    """one call, one segment per (digest array, index list); the outputs are columns of one arena, each as long as the longest list"""
    n = len(srcs)
    S = [Buf(pl, s) for s in srcs]
    out = Arena(pl, n, 4 * max(len(i) for i in idxs))
    allidx = np.ascontiguousarray(np.concatenate(idxs), dtype=np.uint64)
    rc = pl.lib.ms_gather_digests_multi(pl.handle, n, (VP * n)(*[s.ptr for s in S]), (SZ * n)(*[s.size // 4 for s in srcs]), allidx.ctypes.data,
                                        (SZ * n)(*[len(i) for i in idxs]), (VP * n)(*out.ptrs))
    assert rc == MS_OK, pl.lib.ms_last_error()
    want = np.full((n, out.stride), JUNK, dtype=np.uint64)
    for s, (src, idx) in enumerate(zip(srcs, idxs)):
        want[s, :4 * len(idx)] = src.reshape(-1, 4)[idx.astype(np.int64)].reshape(-1)
    same(out.buf.read(), want.reshape(-1), what)
    for buf, src in zip(S, srcs):
        same(buf.read(), src, what + ": the digests")


def digest_indices(ndigests, count, seed):
    return positions_for(ndigests, count, seed)


LONG_COUNT = (1 << 18) + 3              # * 4 words > 2^20; 2 MiB of indices: more than a slot of the staging ring


@pytest.mark.parametrize("kind", KINDS)
def test_gather_digests_past_the_grid_cap(kind):
    assert LONG_COUNT * 4 > CAP
    gather_single(backends.planner(kind), words(FP, 4 * 1024, 21), digest_indices(1024, LONG_COUNT, 22), "2^18 + 3 of 1024 digests")


@pytest.mark.parametrize("kind", KINDS)
def test_gather_digests_multi_past_the_grid_cap(kind):
    gather_multi(backends.planner(kind), [words(FP, 4 * 1024, 23), words(FP, 4 * 16, 24)], [digest_indices(1024, LONG_COUNT, 25), digest_indices(16, 77, 26)],
                 "two segments, 2^18 + 3 and 77 records")


@pytest.mark.parametrize("kind", KINDS)
def test_gather_digests_of_252_bit_elements(kind):
    """a 32-byte record is one element of the 252-bit field (the rows of its FRI layers are gathered this way); short lists, one digest, an empty segment"""
    pl = backends.planner(kind)
    col = M252.values(300, 31)
    for count in (1, 2, 47, 300, 1025):
        gather_single(pl, col, digest_indices(300, count, count), f"{count} elements of a 252-bit column")
    gather_single(pl, col[:4], np.zeros(5, dtype=np.uint64), "one digest, five times")
    gather_multi(pl, [col, M252.values(2, 32), col[:4 * 77]], [digest_indices(300, 90, 33), np.array([], dtype=np.uint64), digest_indices(77, 513, 34)],
                 "three segments of 252-bit elements, the second empty")


# ------------------------------------------------------------------------------------------------------------------
# aliasing: an output over a source or over another output is refused before anything is enqueued
# ------------------------------------------------------------------------------------------------------------------
def _refused():
    """(name, call(L, h, base) -> rc) on one arena of 4096 words; addresses are byte offsets from its start"""
    pos = np.array([3, 0, 9, 9], dtype=np.uint64)
    out = []

    def rows(field, where):
        def call(L, h, b):
            v = V[field]
            cols = (VP * 2)(b + 1024, b + 1024 + 8 * 16 * v)                                  # two columns of 16 rows
            return L.ms_gather_rows(h, field, 16, cols, 2, pos.ctypes.data, 4, b + 1024 + where(v))
        return call
    for f in FIELDS:
        out.append((f"ms_gather_rows {FNAME[f]}: the output starts in the last word of column 1", rows(f, lambda v: 8 * 32 * v - 8)))
        out.append((f"ms_gather_rows {FNAME[f]}: the output ends in the first word of column 0", rows(f, lambda v: -8 * 4 * 2 * v + 8)))
        out.append((f"ms_gather_rows {FNAME[f]}: the output is column 0", rows(f, lambda v: 0)))
    idx = np.array([1, 0, 7, 7, 2], dtype=np.uint64)

    def single(where):
        return lambda L, h, b: L.ms_gather_digests(h, 8, b + 1024, idx.ctypes.data, 5, b + 1024 + where)
    out.append(("ms_gather_digests: the output starts inside the digest array", single(32 * 3)))
    out.append(("ms_gather_digests: the output is the digest array", single(0)))
    out.append(("ms_gather_digests: the output ends in the first digest", single(-32 * 5 + 8)))

    def multi(outs):
        def call(L, h, b):
            srcs = (VP * 2)(b + 1024, b + 4096)                                                 # 8 digests each
            return L.ms_gather_digests_multi(h, 2, srcs, (SZ * 2)(8, 8), idx.ctypes.data, (SZ * 2)(3, 2), (VP * 2)(*[b + o for o in outs]))
        return call
    out.append(("ms_gather_digests_multi: the output of segment 0 starts inside the digests of segment 1", multi((4096 + 32 * 7, 8192))))
    out.append(("ms_gather_digests_multi: the output of segment 1 is inside its own digests", multi((8192, 4096 + 64))))
    out.append(("ms_gather_digests_multi: the two outputs overlap", multi((8192, 8192 + 32 * 2))))
    out.append(("ms_gather_digests_multi: the two outputs are the same", multi((8192, 8192))))

    def deint(field, outs):
        def call(L, h, b):
            v = V[field]
            return L.ms_deinterleave(h, field, 10, 3, b + 1024, (VP * 3)(*[b + o(v) for o in outs]))   # d_in: 30 elements at +1024
        return call
    for f in FIELDS:
        far = [lambda v: 8192, lambda v: 12288, lambda v: 16384]
        out.append((f"ms_deinterleave {FNAME[f]}: column 1 starts in the last word of d_in", deint(f, [far[0], lambda v: 1024 + 8 * 30 * v - 8, far[2]])))
        out.append((f"ms_deinterleave {FNAME[f]}: column 0 is d_in", deint(f, [lambda v: 1024, far[1], far[2]])))
        out.append((f"ms_deinterleave {FNAME[f]}: column 2 ends in the first word of d_in", deint(f, [far[0], far[1], lambda v: 1024 - 8 * 10 * v + 8])))
        out.append((f"ms_deinterleave {FNAME[f]}: columns 0 and 2 overlap by a word", deint(f, [far[0], far[1], lambda v: 8192 + 8 * 10 * v - 8])))
        out.append((f"ms_deinterleave {FNAME[f]}: columns 1 and 2 are the same", deint(f, [far[0], far[1], far[1]])))
    return out


REFUSED = _refused()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", range(len(REFUSED)), ids=[name.replace(" ", "_").replace(":", "") for name, _ in REFUSED])
def test_overlapping_buffers_are_refused(kind, shape):
    pl = backends.planner(kind)
    before = np.random.default_rng(3).integers(0, 1 << 64, size=4096, dtype=np.uint64)
    arena = Buf(pl, before)
    name, call = REFUSED[shape]
    rc = call(pl.lib, pl.handle, arena.ptr)
    msg = pl.lib.ms_last_error().decode()
    assert rc == MS_ERR_INVALID, f"{name}: returned {rc}"          # stop here: the words of an accepted call are never looked at
    assert "overlap" in msg and name.split(" ")[0].rstrip(":") in msg, msg
    pl.sync()
    same(arena.read(), before, "the arena after a refused call")


@pytest.mark.parametrize("kind", KINDS)
def test_touching_buffers_and_empty_calls_are_allowed(kind):
    """an output that starts where a source ends is disjoint from it; an empty segment and an empty position list are exempt from the rule"""
    pl = backends.planner(kind)
    L, h = pl.lib, pl.handle
    for field in FIELDS:
        v = V[field]
        src = words(field, 30, 40 + field)
        junk = np.full(30 * v, JUNK, dtype=np.uint64)
        X = Buf(pl, np.concatenate([src, junk]))                                # d_in | column 0 | column 1 | column 2
        base = X.ptr + 8 * 30 * v
        assert L.ms_deinterleave(h, field, 10, 3, X.ptr, (VP * 3)(base, base + 80 * v, base + 160 * v)) == MS_OK, L.ms_last_error()
        same(X.read(), np.concatenate([src, src.reshape(10, 3, v).transpose(1, 0, 2).reshape(-1)]), "adjacent columns behind d_in")
        pos = np.array([9, 0, 9], dtype=np.uint64)
        X = Buf(pl, np.concatenate([src, junk]))                                # columns 0, 1, 2 of 10 rows | the 3 gathered rows
        base = X.ptr + 8 * 30 * v
        assert L.ms_gather_rows(h, field, 10, (VP * 3)(X.ptr, X.ptr + 80 * v, X.ptr + 160 * v), 3, pos.ctypes.data, 3, base) == MS_OK, L.ms_last_error()
        got = X.read()
        same(got[:30 * v], src, "the columns")
        same(got[30 * v:39 * v], src.reshape(3, 10, v)[:, [9, 0, 9], :].transpose(1, 0, 2).reshape(-1), "rows gathered right behind the columns")
        same(got[39 * v:], junk[9 * v:], "behind the gathered rows")
        assert L.ms_gather_rows(h, field, 10, (VP * 3)(X.ptr, X.ptr + 80 * v, X.ptr + 160 * v), 3, pos.ctypes.data, 0, X.ptr) == MS_OK     # no position
    dig = words(FP, 4 * 8, 50)
    junk = np.full(4 * 8, JUNK, dtype=np.uint64)
    idx = np.array([7, 0, 7], dtype=np.uint64)
    X = Buf(pl, np.concatenate([dig, junk]))
    assert L.ms_gather_digests(h, 8, X.ptr, idx.ctypes.data, 3, X.ptr + 256) == MS_OK, L.ms_last_error()
    assert L.ms_gather_digests(h, 8, X.ptr, idx.ctypes.data, 0, X.ptr) == MS_OK                                                         # no index
    # segment 1 is empty: its pointers are not looked at; segment 2 writes right behind segment 0's output
    rc = L.ms_gather_digests_multi(h, 3, (VP * 3)(X.ptr, X.ptr, X.ptr), (SZ * 3)(8, 8, 8), np.array([1, 2, 3], dtype=np.uint64).ctypes.data, (SZ * 3)(2, 0, 1),
                                   (VP * 3)(X.ptr + 256 + 96, X.ptr, X.ptr + 256 + 160))
    assert rc == MS_OK, L.ms_last_error()
    d = dig.reshape(8, 4)
    same(X.read(), np.concatenate([dig, d[7], d[0], d[7], d[1], d[2], d[3], junk[24:]]), "digests gathered right behind their array")
