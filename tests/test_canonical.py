"""The canonical-form scan (ms_check_canonical, ms_check_canonical_host) and the checked mode built on it (ms_ctx_set_checked).  Every device
test runs on the simulator build and, marked gpu, on the device.  What a scan must report is worked out here from Python integers and from
where the test planted its values; nothing shares code with csrc/.

  1  clean data: every length and column count, edge values that are just canonical, columns compared with their upload afterwards
  2  planted values: every non-canonical shape, at the rows, columns and alignments where the kernel changes its path
  3  the host scan over the same values
  4  checked mode, one case per entry point and field (CASES): the refusal names argument, column and row, nothing is written, and clean
     input gives the unchecked words bit for bit
  5  every ms_* name of the header is classified (CLASSES); every `checks` name is reached by a case of 4
  6  the default, and MS_CHECK_CANONICAL in the environment
  7  the Python mirror (the C++ one: tests/test_canonical_mirror.py)
  8  rate, device only: the scan of 8 Fp columns of 2^24 elements takes no longer than eight ms_unary(MS_NEG) calls over the same buffers"""
import collections
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import backends
from tests.test_stage_sweep import GUARD, M252, Buf, same
from tests.deep_ref import B252, FP, FQ3, F252, G, MS_ERR_INVALID, MS_OK, P, P252, PW, VP, call_deep, call_horner, u64
from tests.test_deep_sweep import Rows, rows_inputs
from ministark_amd import Matrix, Planner, _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = (FP, FQ3, F252)
FNAME = {FP: "fp", FQ3: "fq3", F252: "f252"}
P3 = 0x0800000000000011                 # limb 3 of p252 = 2^251 + 17 * 2^192 + 1
M64 = (1 << 64) - 1
assert P == (1 << 64) - (1 << 32) + 1 and P252 == (1 << 251) + 17 * (1 << 192) + 1 and P252 >> 192 == P3
NS = [0, 1, 2, 63, 64, 65, 255, 257, 4095, 4096, 4097, (1 << 16) + 3]
NCOLS = [0, 1, 3, 8, 97]
# just canonical: must not be flagged
GL_OK = [P - 1, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF]
F252_OK = [P252 - 1, P3 << 192, ((P3 - 1) << 192) | ((1 << 192) - 1)]
# not canonical
GL_BAD = [P, P + 1, M64]
F252_BAD = [P252, P252 + 1, (1 << 256) - 1, (P3 + 1) << 192, (P3 << 192) | (5 << 64)]
assert all(v < P for v in GL_OK) and all(v >= P for v in GL_BAD) and all(v < P252 for v in F252_OK) and all(v >= P252 for v in F252_BAD)


def limbs(x):
    return [(x >> (64 * k)) & M64 for k in range(4)]


def clean_words(field, n, seed):
    """n canonical elements: uniform, with the just-canonical edge values at the ends and sprinkled between"""
    rng = np.random.default_rng(seed)
    v = PW[field]
    if field == F252:
        a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        a[:, 3] = rng.integers(0, P3, size=n, dtype=np.uint64)
        edge = np.array([limbs(x) for x in F252_OK], dtype=np.uint64)
        m = rng.random(n) < 0.05
        a[m] = edge[rng.integers(0, len(edge), size=int(m.sum()))]
        for i, x in enumerate(F252_OK):
            if n > 2 * i + 1:
                a[i], a[n - 1 - i] = edge[i], edge[(i + 1) % 3]
        return np.ascontiguousarray(a.reshape(-1))
    a = rng.integers(0, P, size=n * v, dtype=np.uint64)
    edge = np.array(GL_OK, dtype=np.uint64)
    m = rng.random(n * v) < 0.05
    a[m] = edge[rng.integers(0, len(edge), size=int(m.sum()))]
    for i in range(min(3, (n * v) // 2)):
        a[i], a[n * v - 1 - i] = edge[i], edge[(i + 1) % 3]
    return a


def is_bad(field, w):
    """one element's words -> index of its first non-canonical component, or None (Python integers)"""
    if field == F252:
        return 0 if sum(int(x) << (64 * k) for k, x in enumerate(w)) >= P252 else None
    return next((k for k, x in enumerate(w) if int(x) >= P), None)


def py_report(field, cols):
    """(count, first_col, first_row, first_word) of a list of word arrays, element by element in Python integers"""
    v, count, first = PW[field], 0, None
    for c, col in enumerate(cols):
        for r in range(col.size // v):
            k = is_bad(field, col[r * v:(r + 1) * v])
            if k is not None:
                count += 1
                first = first or (c, r, k)
    return (count,) + (first or (0, 0, 0))


def scan(pl, field, n, ptrs, ncols=None):
    rep = _lib.CanonReport()
    tab = (VP * max(1, len(ptrs)))(*ptrs)
    rc = pl.lib.ms_check_canonical(pl.handle, field, n, tab, len(ptrs) if ncols is None else ncols, ctypes.byref(rep))
    assert rc == MS_OK, pl.lib.ms_last_error().decode()
    return rep


def as_tuple(rep):
    return (rep.count, rep.first_col, rep.first_row, rep.first_word) if rep.count else (0, 0, 0, 0)


def plant(field, col, row, value, comp=0):
    """write a value (an integer: one word, or for the 252-bit field the whole element) into a word array"""
    if field == F252:
        col[4 * row:4 * row + 4] = limbs(value)
    else:
        col[PW[field] * row + comp] = value


# ---------------------------------------------------------------------------------------------------------------------------------
# 1  clean data
# ---------------------------------------------------------------------------------------------------------------------------------
CLEAN = [pytest.param(k, f, n, nc, id=f"{k}-{FNAME[f]}-n{n}-c{nc}", marks=[pytest.mark.gpu] if k == "hip" else [])
         for k in ("emu", "hip") for f in FIELDS for n in NS for nc in NCOLS]
CLEAN += [pytest.param(k, f, 64, 4100, id=f"{k}-{FNAME[f]}-n64-c4100", marks=[pytest.mark.gpu] if k == "hip" else []) for k in ("emu", "hip") for f in FIELDS]
CLEAN += [pytest.param("hip", f, 1 << 24, nc, id=f"hip-{FNAME[f]}-n16777216-c{nc}", marks=pytest.mark.gpu) for f in FIELDS for nc in (1, 3)]


@pytest.mark.parametrize("kind,field,n,ncols", CLEAN)
def test_scan_clean(kind, field, n, ncols):
    pl = backends.planner(kind)
    distinct = min(ncols, 8) if n >= 1 << 20 or ncols > 1000 else ncols          # beyond that the columns alias each other (they may)
    words = [clean_words(field, n, 100 * n + c) for c in range(distinct)]
    bufs = [Buf(pl, w) for w in words]
    ptrs = [bufs[c % distinct].ptr for c in range(ncols)]
    rep = scan(pl, field, n, ptrs)
    assert rep.count == 0 and bool(rep), rep
    for b, w in zip(bufs, words):
        same(b.read(), w, "a column after the scan")


@pytest.mark.parametrize("kind", KINDS)
def test_scan_arguments(kind):
    pl = backends.planner(kind)
    L, rep = pl.lib, _lib.CanonReport()
    b = Buf(pl, clean_words(FP, 16, 1))
    tab = (VP * 2)(b.ptr, None)
    assert L.ms_check_canonical(pl.handle, 7, 16, tab, 1, ctypes.byref(rep)) == MS_ERR_INVALID
    assert L.ms_check_canonical(pl.handle, FP, 16, None, 1, ctypes.byref(rep)) == MS_ERR_INVALID
    assert L.ms_check_canonical(pl.handle, FP, 16, tab, 2, ctypes.byref(rep)) == MS_ERR_INVALID and "column 1" in L.ms_last_error().decode()
    assert L.ms_check_canonical(pl.handle, FP, 16, tab, 1, None) == MS_ERR_INVALID
    assert L.ms_check_canonical(pl.handle, FP, 0, tab, 2, ctypes.byref(rep)) == MS_OK and rep.count == 0       # n = 0: the columns are not looked at
    assert L.ms_check_canonical(pl.handle, FP, 16, None, 0, ctypes.byref(rep)) == MS_OK and rep.count == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2  planted values
# ---------------------------------------------------------------------------------------------------------------------------------
def bad_values(field):
    return F252_BAD if field == F252 else GL_BAD


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
def test_every_bad_value_in_every_component(kind, field):
    pl = backends.planner(kind)
    n, v = 300, PW[field]
    for value in bad_values(field):
        for comp in range(v if field == FQ3 else 1):
            w = clean_words(field, n, 5)
            plant(field, w, 123, value, comp)
            b = Buf(pl, w)
            assert as_tuple(scan(pl, field, n, [b.ptr])) == (1, 0, 123, comp), (hex(value), comp)
            same(b.read(), w, "the column after the scan")
    if field == FQ3:            # two bad components: one element, the lower component is reported
        for lo, hi in ((0, 1), (0, 2), (1, 2)):
            w = clean_words(field, n, 6)
            plant(field, w, 77, P, hi)
            plant(field, w, 77, M64, lo)
            assert as_tuple(scan(pl, field, n, [Buf(pl, w).ptr])) == (1, 0, 77, lo)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
def test_first_and_last_row_at_every_ragged_length(kind, field):
    pl = backends.planner(kind)
    for n in NS[1:]:
        for row in {0, n - 1}:
            value = bad_values(field)[(n + row) % len(bad_values(field))]
            comp = (n + row) % 3 if field == FQ3 else 0
            w = clean_words(field, n, n)
            plant(field, w, row, value, comp)
            assert as_tuple(scan(pl, field, n, [Buf(pl, w).ptr])) == (1, 0, row, comp), (n, row)
            # the same column one element into its allocation: the pointer is element-aligned only (an 8-byte-aligned head for Fp)
            arena = Buf(pl, np.concatenate([clean_words(field, 1, 9), w]))
            assert arena.ptr % 16 == 0
            assert as_tuple(scan(pl, field, n, [arena.ptr + 8 * PW[field]])) == (1, 0, row, comp), (n, row, "shifted")
            if field != FP:     # ... and one WORD in: the 8-byte-aligned head of a wide element
                arena = Buf(pl, np.concatenate([u64([M64]), w, u64([M64])]))
                assert as_tuple(scan(pl, field, n, [arena.ptr + 8])) == (1, 0, row, comp), (n, row, "one word in")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
def test_unaligned_head_and_tail_words_are_not_read_past(kind, field):
    """bad words directly before and behind a clean column that starts 8 bytes off a 16-byte boundary: not the column's, not reported"""
    pl = backends.planner(kind)
    for n in (1, 2, 63, 64, 1024, 4097):
        w = clean_words(field, n, n + 1)
        arena = Buf(pl, np.concatenate([u64([M64]), w, u64([M64, M64])]))
        assert scan(pl, field, n, [arena.ptr + 8]).count == 0, n
        arena = Buf(pl, np.concatenate([u64([M64, M64]), w, u64([M64, M64])]))
        assert scan(pl, field, n, [arena.ptr + 16]).count == 0, n


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
def test_columns(kind, field):
    pl = backends.planner(kind)
    n, bad = 4097, bad_values(field)
    words = [clean_words(field, n, 40 + c) for c in range(8)]
    plant(field, words[5], 2048, bad[0], PW[field] - 1 if field == FQ3 else 0)
    bufs = [Buf(pl, w) for w in words]
    assert as_tuple(scan(pl, field, n, [b.ptr for b in bufs])) == (1, 5, 2048, 2 if field == FQ3 else 0)
    # columns 2 and 6: column 2 is reported although its row is the larger one
    words = [clean_words(field, n, 50 + c) for c in range(8)]
    plant(field, words[2], 4000, bad[1])
    plant(field, words[6], 3, bad[2])
    bufs = [Buf(pl, w) for w in words]
    assert as_tuple(scan(pl, field, n, [b.ptr for b in bufs])) == (2, 2, 4000, 0)
    # aliasing: the bad column listed three times counts three times
    assert as_tuple(scan(pl, field, n, [bufs[0].ptr, bufs[6].ptr, bufs[6].ptr, bufs[1].ptr, bufs[6].ptr])) == (3, 1, 3, 0)
    # beyond one launch's pointer table: the only bad column is number 4099 of 4100
    short = [Buf(pl, clean_words(field, 64, 60)), None]
    w = clean_words(field, 64, 61)
    plant(field, w, 63, bad[0])
    short[1] = Buf(pl, w)
    assert as_tuple(scan(pl, field, 64, [short[0].ptr] * 4099 + [short[1].ptr])) == (1, 4099, 63, 0)
    assert as_tuple(scan(pl, field, 64, [short[0].ptr] * 7 + [short[1].ptr] + [short[0].ptr] * 4090 + [short[1].ptr] * 2)) == (3, 7, 63, 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
@pytest.mark.parametrize("k", [1, 7, 1000])
def test_random_plants(kind, field, k):
    pl = backends.planner(kind)
    n, ncols, v, bad = 4097, 8, PW[field], bad_values(field)
    rng = np.random.default_rng(1000 * field + k)
    words = [clean_words(field, n, 70 + c) for c in range(ncols)]
    for _ in range(k):          # plants may fall on one element twice, in one component or in two
        plant(field, words[int(rng.integers(ncols))], int(rng.integers(n)), bad[int(rng.integers(len(bad)))], int(rng.integers(v)) if field == FQ3 else 0)
    want = py_report(field, words)
    assert 0 < want[0] <= k
    bufs = [Buf(pl, w) for w in words]
    assert as_tuple(scan(pl, field, n, [b.ptr for b in bufs])) == want
    for b, w in zip(bufs, words):
        same(b.read(), w, "a column after the scan")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3  the host scan (no context, no device: the simulator build's library serves)
# ---------------------------------------------------------------------------------------------------------------------------------
def host_scan(L, field, w, count=None):
    first = ctypes.c_size_t(12345)
    count = w.size // PW[field] if count is None else count
    assert L.ms_check_canonical_host(field, w.ctypes.data if w.size else None, count, ctypes.byref(first)) == MS_OK
    return first.value


@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
def test_host_scan(field):
    L = backends.planner("emu").lib
    assert host_scan(L, field, np.zeros(0, dtype=np.uint64)) == 0                        # count = 0
    for n in (1, 2, 65, 4097):
        w = clean_words(field, n, n)
        assert host_scan(L, field, w) == n
        for value in bad_values(field):
            for comp in range(3 if field == FQ3 else 1):
                for row in {0, n // 2, n - 1}:
                    x = w.copy()
                    plant(field, x, row, value, comp)
                    plant(field, x, n - 1, value, comp)
                    assert host_scan(L, field, x) == row, (n, hex(value), comp, row)
    first = ctypes.c_size_t(0)
    assert L.ms_check_canonical_host(9, None, 0, ctypes.byref(first)) == MS_ERR_INVALID
    assert L.ms_check_canonical_host(field, None, 1, ctypes.byref(first)) == MS_ERR_INVALID
    assert L.ms_check_canonical_host(field, clean_words(field, 1, 1).ctypes.data, 1, None) == MS_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------------------------
# 4  checked mode
# ---------------------------------------------------------------------------------------------------------------------------------
# An argument of a case.  kind "dev": `cols` = word arrays of n elements each (uploaded one buffer per column; the call sees their pointers);
# "mat": one row-major matrix [n][ncols]; "host": `cols[0]` = packed host elements (row = element index * row_scale).
Arg = collections.namedtuple("Arg", "name kind field cols ncols row_scale", defaults=(1, 1))
Case = collections.namedtuple("Case", "entries field tag make")
LOG = 6
N = 1 << LOG


def dev(name, field, n, ncols, seed):
    return Arg(name, "dev", field, [clean_words(field, n, seed + c) for c in range(ncols)])


def host(name, field, count, seed, row_scale=1):
    return Arg(name, "host", field, [clean_words(field, count, seed)], 1, row_scale)


def mont(field, x):
    return M252.words([B252.to_mont(x)]) if field == F252 else u64([G.to_mont(x)])


def base_of(field):
    return F252 if field == F252 else FP


def table(ptrs):
    return (VP * max(1, len(ptrs)))(*ptrs)


def hp(a):
    return a.ctypes.data


def _ntt_cases():
    def plan_create(field):
        def make(pl):
            bf = base_of(field)
            F = B252 if field == F252 else G
            args = [Arg("h_offset", "host", bf, [mont(field, 5)]), Arg("h_group_gen", "host", bf, [mont(field, F.root_of_unity(N))])]

            def call(A, O):
                h = VP()
                rc = pl.lib.ms_ntt_plan_create(pl.handle, field, LOG, 0, hp(A["h_offset"]), hp(A["h_group_gen"]), ctypes.byref(h))
                if rc == MS_OK:
                    pl.lib.ms_ntt_plan_destroy(h)
                return rc
            return args, [], call
        return make

    def transform(field, how):
        def make(pl):
            name = {"enqueue": "d_columns", "enqueue_to": "d_src", "execute": "d_column"}[how]
            args = [dev(name, field, N, 3, 11)]
            outs = [np.full(N * PW[field], 0x7777, dtype=np.uint64) for _ in range(3)] if how == "enqueue_to" else []

            def call(A, O):
                h = VP()
                assert pl.lib.ms_ntt_plan_create(pl.handle, field, LOG, 0, None, None, ctypes.byref(h)) == MS_OK
                try:
                    if how == "enqueue":
                        return pl.lib.ms_ntt_enqueue(h, table(A[name]), 3)
                    if how == "enqueue_to":
                        return pl.lib.ms_ntt_enqueue_to(h, table(A[name]), table(O), 3)
                    for p in A[name]:
                        assert pl.lib.ms_ntt_encode(h, p) == MS_OK
                    return pl.lib.ms_ntt_execute(h)
                finally:
                    pl.lib.ms_ntt_plan_destroy(h)
            return args, outs, call
        return make
    out = []
    for f in FIELDS:
        out.append(Case(("ms_ntt_plan_create",), f, "", plan_create(f)))
        out.append(Case(("ms_ntt_enqueue",), f, "in-place", transform(f, "enqueue")))
        out.append(Case(("ms_ntt_enqueue_to",), f, "", transform(f, "enqueue_to")))
        out.append(Case(("ms_ntt_encode", "ms_ntt_execute"), f, "in-place", transform(f, "execute")))
    return out


def _lde_cases():
    def lde(field, entry):
        def make(pl):
            args = [dev("d_in", field, N, 2, 21), Arg("h_offset", "host", base_of(field), [mont(field, 3 if field == F252 else 7)])]
            outs = [np.full(4 * N * PW[field], 0x5555, dtype=np.uint64) for _ in range(2)]

            def call(A, O):
                if entry == "ms_lde":
                    return pl.lib.ms_lde(pl.handle, field, LOG, 2, hp(A["h_offset"]), table(A["d_in"]), table(O), 2, 1)
                return pl.lib.ms_evaluate(pl.handle, field, LOG, LOG + 2, hp(A["h_offset"]), table(A["d_in"]), table(O), 2, 0)
            return args, outs, call
        return make
    return [Case((e,), f, "", lde(f, e)) for f in FIELDS for e in ("ms_lde", "ms_evaluate")]


def _stage_cases():
    n = 300
    L = lambda pl: pl.lib

    def binary(lf, rf, entry):
        def make(pl):
            args = [dev("d_lhs", lf, n, 1, 31), dev("d_rhs", rf, n, 1, 32)]
            outs = [np.full(n * PW[lf], 0x1234, dtype=np.uint64)]
            if entry == "ms_binary":
                call = lambda A, O: L(pl).ms_binary(pl.handle, 1, lf, rf, n, O[0], A["d_lhs"][0], A["d_rhs"][0], 5)
            else:
                call = lambda A, O: L(pl).ms_mul_pow(pl.handle, lf, rf, n, O[0], A["d_lhs"][0], A["d_rhs"][0], 3, -2)
            return args, outs, call
        return make

    def const(lf, rf):
        def make(pl):
            args = [dev("d_lhs", lf, n, 1, 33), host("h_const", rf, 1, 34)]
            return args, [], lambda A, O: L(pl).ms_binary_const(pl.handle, 0, lf, rf, n, A["d_lhs"][0], A["d_lhs"][0], hp(A["h_const"]))     # AddAssignConst
        return make

    def unary(f, op, inplace):
        def make(pl):
            args = [dev("d_src", f, n, 1, 35)]
            if inplace:
                return args, [], lambda A, O: L(pl).ms_unary(pl.handle, op, f, n, A["d_src"][0], A["d_src"][0], 5)
            return args, [np.full(n * PW[f], 0x4321, dtype=np.uint64)], lambda A, O: L(pl).ms_unary(pl.handle, op, f, n, O[0], A["d_src"][0], 5)
        return make

    def convert(df, sf):
        def make(pl):
            return [dev("d_src", sf, n, 1, 36)], [np.full(n * PW[df], 0x99, dtype=np.uint64)], lambda A, O: L(pl).ms_convert(pl.handle, df, sf, n, O[0], A["d_src"][0])
        return make

    def fill(f):
        def make(pl):
            return [host("h_value", f, 1, 37)], [np.full(n * PW[f], 0x98, dtype=np.uint64)], lambda A, O: L(pl).ms_fill(pl.handle, f, n, O[0], hp(A["h_value"]))
        return make

    def sumc(f):
        def make(pl):
            return ([dev("d_cols", f, n, 4, 38)], [np.full(n * PW[f], 0x97, dtype=np.uint64)],
                    lambda A, O: L(pl).ms_sum_columns(pl.handle, f, n, table(A["d_cols"]), 4, O[0]))
        return make
    out = []
    for lf, rf in ((FP, FP), (FQ3, FQ3), (FQ3, FP), (F252, F252)):
        tag = FNAME[rf] + "-rhs"
        out += [Case(("ms_binary",), lf, tag, binary(lf, rf, "ms_binary")), Case(("ms_mul_pow",), lf, tag, binary(lf, rf, "ms_mul_pow")),
                Case(("ms_binary_const",), lf, tag + "-in-place", const(lf, rf))]
    for f in FIELDS:
        out += [Case(("ms_unary",), f, "neg-in-place", unary(f, 0, True)), Case(("ms_unary",), f, "exp-into", unary(f, 2, False)),
                Case(("ms_convert",), f, "copy", convert(f, f)), Case(("ms_fill",), f, "", fill(f)), Case(("ms_sum_columns",), f, "", sumc(f))]
    out.append(Case(("ms_convert",), FQ3, "embed-fp", convert(FQ3, FP)))
    return out


def _hash_cases():
    n = 130

    def rows(entry, f, with_field):
        def make(pl):
            fn = getattr(pl.lib, entry)
            head = (pl.handle, f, n) if with_field else (pl.handle, n)
            return [dev("d_cols", f, n, 3, 41)], [np.full(4 * n, 0x61, dtype=np.uint64)], lambda A, O: fn(*head, table(A["d_cols"]), 3, O[0])
        return make

    def rowmajor(entry, f, with_field, ncols):
        def make(pl):
            fn = getattr(pl.lib, entry)
            head = (pl.handle, f, n, ncols) if with_field else (pl.handle, n, ncols)
            return ([Arg("d_matrix", "mat", f, [clean_words(f, n * ncols, 42)], ncols)], [np.full(4 * n, 0x62, dtype=np.uint64)],
                    lambda A, O: fn(*head, A["d_matrix"][0], O[0]))
        return make

    def merkle(pl):
        return ([Arg("d_leaves", "mat", FP, [clean_words(FP, 4 * 64, 43)], 4)], [np.full(4 * 64, 0x63, dtype=np.uint64)],
                lambda A, O: pl.lib.ms_rpo256_merkle(pl.handle, 64, A["d_leaves"][0], O[0]))
    out = []
    for f in FIELDS:
        out += [Case(("ms_sha256_rows",), f, "", rows("ms_sha256_rows", f, True)), Case(("ms_blake2s_rows",), f, "", rows("ms_blake2s_rows", f, True)),
                Case(("ms_sha256_rows_row_major",), f, "", rowmajor("ms_sha256_rows_row_major", f, True, 5)),
                Case(("ms_blake2s_rows_row_major",), f, "", rowmajor("ms_blake2s_rows_row_major", f, True, 5))]
    out += [Case(("ms_rpo256_rows",), FP, "", rows("ms_rpo256_rows", FP, False)), Case(("ms_rpo256_rows_row_major",), FP, "", rowmajor("ms_rpo256_rows_row_major", FP, False, 8)),
            Case(("ms_rpo256_rows_field",), FP, "", rows("ms_rpo256_rows_field", FP, True)), Case(("ms_rpo256_rows_field",), FQ3, "", rows("ms_rpo256_rows_field", FQ3, True)),
            Case(("ms_rpo256_merkle",), FP, "", merkle)]
    return out


OP = dict(X_P=0, CONST_P=1, CONST_Q=2, TRACE_P=3, TRACE_Q=4, PERIODIC_P=5, NEG_P=7, ADD_PP=9, ADD_QP=11, MUL_PP=12, MUL_QQ=13, STORE_Q=20, STORE_P=21)


def _program(field):
    """(x_i + base0 * const + periodic0) [over Fq3: + ext0 * const_q] stored as constraint / output 0; the constants' word offsets"""
    pw = 4 if field == F252 else 1
    prog = [(OP["TRACE_P"], 0, 0, 0), (OP["CONST_P"], 1, 0, 0), (OP["MUL_PP"], 2, 0, 1), (OP["X_P"], 3, 0, 0), (OP["ADD_PP"], 4, 2, 3),
            (OP["PERIODIC_P"], 5, 0, 0), (OP["ADD_PP"], 6, 4, 5)]
    if field == FQ3:
        prog += [(OP["TRACE_Q"], 0, 0, 0), (OP["CONST_Q"], 1, pw, 0), (OP["MUL_QQ"], 2, 0, 1), (OP["ADD_QP"], 3, 2, 6), (OP["STORE_Q"], 0, 3, 0)]
    else:
        prog += [(OP["STORE_P"], 0, 6, 0)]
    return np.array(prog, dtype=np.uint32).reshape(-1)


def _eval_cases():
    def make_for(field, entry):
        def make(pl):
            bf = base_of(field)
            prog = _program(field)
            ninstr = prog.size // 4
            if field == F252:
                consts = host("h_consts", F252, 1, 51, row_scale=4)
            else:
                consts = host("h_consts", FP, 4 if field == FQ3 else 1, 51)          # Goldilocks constants are checked word by word
            nwords = consts.cols[0].size
            args = [consts, dev("d_base_cols", bf, N, 2, 52), dev("d_periodic", bf, 8, 1, 54)]
            if field == FQ3:
                args.append(dev("d_ext_cols", FQ3, N, 2, 53))
            plen = (ctypes.c_uint * 1)(8)
            if entry == "ms_validate_constraints":
                outs = [np.full(2, 0xAB, dtype=np.uint64)]                           # h_first_row | h_rows_failed: host memory, passed as is

                def call(A, O):
                    ext = A.get("d_ext_cols", [])
                    return pl.lib.ms_validate_constraints(pl.handle, bf, hp(prog), ninstr, hp(A["h_consts"]), nwords, LOG, table(A["d_base_cols"]), 2,
                                                          table(ext), len(ext), table(A["d_periodic"]), plen, 1, 1, O[0], O[0] + 8)
                return args, outs, call
            args += [Arg("h_domain_offset", "host", bf, [mont(field, 3 if field == F252 else 7)]), dev("d_x_lde", bf, N, 1, 55)]
            outs = [np.full(N * PW[field], 0xCD, dtype=np.uint64)]

            def call(A, O):
                ext = A.get("d_ext_cols", [])
                a = (pl.handle, hp(prog), ninstr, hp(A["h_consts"]), nwords, LOG, 1, hp(A["h_domain_offset"]), A["d_x_lde"][0], table(A["d_base_cols"]), 2,
                     table(ext), len(ext), table(A["d_periodic"]), plen, 1, field, O[0])
                return pl.lib.ms_eval_program(*a) if entry == "ms_eval_program" else pl.lib.ms_eval_program_ex(*a, 2)
            return args, outs, call
        return make
    return [Case((e,), f, "", make_for(f, e)) for f in FIELDS for e in ("ms_eval_program", "ms_eval_program_ex", "ms_validate_constraints")]


def _scan_fri_cases():
    n = 1000

    def scan_affine(f):
        def make(pl):
            return ([dev("d_a", f, n, 1, 61), dev("d_b", f, n, 1, 62), host("h_init", f, 1, 63)], [np.full(n * PW[f], 0x31, dtype=np.uint64)],
                    lambda A, O: pl.lib.ms_scan_affine(pl.handle, f, n, A["d_a"][0], A["d_b"][0], hp(A["h_init"]), 1, O[0]))
        return make

    def fold(f, entry):
        def make(pl):
            rows_ = entry == "ms_fri_fold_rows"
            count = 4 * 16 if rows_ else 1 << 8
            args = [dev("d_evals", f, count, 1, 64), host("h_alpha", f, 1, 65), Arg("h_offset", "host", base_of(f), [mont(f, 3 if f == F252 else 7)])]
            outs = [np.full(count // 4 * PW[f], 0x32, dtype=np.uint64)]
            if rows_:
                call = lambda A, O: pl.lib.ms_fri_fold_rows(pl.handle, f, 8, 4, hp(A["h_alpha"]), hp(A["h_offset"]), 5, 16, A["d_evals"][0], O[0])
            else:
                call = lambda A, O: pl.lib.ms_fri_fold(pl.handle, f, 8, 4, hp(A["h_alpha"]), hp(A["h_offset"]), A["d_evals"][0], O[0])
            return args, outs, call
        return make
    return ([Case(("ms_scan_affine",), f, "", scan_affine(f)) for f in FIELDS] +
            [Case((e,), f, "", fold(f, e)) for f in FIELDS for e in ("ms_fri_fold", "ms_fri_fold_rows")])


class _Ptr:
    """what call_deep / call_horner ask of a column: its address"""
    def __init__(self, ptr):
        self.ptr = ptr


def _deep_cases():
    def deep(f, entry):
        def make(pl):
            n = 256
            base, ext, points, tcol, tpoint, alpha, ood, da, db = rows_inputs(Rows(f, 8, 0, n, 3, None, "rand", (), None, None), 5)
            bn, en = ("d_base_rows", "d_ext_rows") if entry == "rows" else ("d_base_polys", "d_ext_polys")
            bf = base_of(f)
            args = [Arg(bn, "dev", bf, base), Arg("h_offset", "host", bf, [mont(f, 3 if f == F252 else 7)]), Arg("h_points", "host", f, [points]),
                    Arg("h_term_alpha", "host", f, [alpha]), Arg("h_term_ood", "host", f, [ood]), Arg("h_degree_alpha", "host", f, [da]), Arg("h_degree_beta", "host", f, [db])]
            if ext:
                args.append(Arg(en, "dev", f, ext))
            head = (lambda A: (8, A["h_offset"], 0, n)) if entry == "rows" else (lambda A: (8, A["h_offset"]))

            def call(A, O):
                return call_deep(pl, entry, f, head(A), [_Ptr(p) for p in A[bn]], [_Ptr(p) for p in A.get(en, [])], A["h_points"], tcol, tpoint,
                                 A["h_term_alpha"], A["h_term_ood"], A["h_degree_alpha"], A["h_degree_beta"], O[0])
            return args, [np.full(n * PW[f], 0x41, dtype=np.uint64)], call
        return make

    def horner(cf, pf):
        def make(pl):
            n = 5000
            args = [dev("d_cols", cf, n, 3, 71), host("h_qpoints", pf, 4, 72)]
            out = np.full(4 * PW[pf], 0x42, dtype=np.uint64)                        # h_out: host memory

            def call(A, O):
                return call_horner(pl, cf, pf, n, [_Ptr(p) for p in A["d_cols"]], [0, 1, 1, 2], A["h_qpoints"], np.ctypeslib.as_array((ctypes.c_uint64 * out.size).from_address(O[0])))
            return args, [out], call
        return make
    out = [Case(("ms_deep_rows",), f, "", deep(f, "rows")) for f in FIELDS] + [Case(("ms_deep_compose",), f, "", deep(f, "compose")) for f in FIELDS]
    out += [Case(("ms_horner_eval",), pf, FNAME[cf] + "-coeffs", horner(cf, pf)) for cf, pf in ((FP, FP), (FP, FQ3), (FQ3, FQ3), (F252, F252))]
    return out


CASES = _ntt_cases() + _lde_cases() + _stage_cases() + _hash_cases() + _eval_cases() + _scan_fri_cases() + _deep_cases()
HOST_OUT = {"ms_validate_constraints", "ms_horner_eval"}        # their results land in host memory


def case_id(c):
    return "+".join(c.entries) + "-" + FNAME[c.field] + ("-" + c.tag if c.tag else "")


class Run:
    """one call of a case: fresh uploads of the (possibly planted) arguments, guard-filled outputs"""
    def __init__(self, pl, case, args, outs):
        self.pl, self.args, self.host_out = pl, args, case.entries[0] in HOST_OUT
        self.bufs = {a.name: [Buf(pl, w) for w in a.cols] for a in args if a.kind != "host"}
        self.host = {a.name: a.cols[0].copy() for a in args if a.kind == "host"}
        self.out_words = outs
        self.outs = [w.copy() for w in outs] if self.host_out else [Buf(pl, w) for w in outs]

    def call(self, fn):
        A = {k: [b.ptr for b in v] for k, v in self.bufs.items()}
        A.update(self.host)
        rc = fn(A, [hp(o) for o in self.outs] if self.host_out else [o.ptr for o in self.outs])
        self.pl.sync()
        return rc

    def read_outs(self):
        return [o.copy() for o in self.outs] if self.host_out else [o.read() for o in self.outs]

    def inputs_unchanged(self, what):
        for a in self.args:
            if a.kind == "host":
                same(self.host[a.name], a.cols[0], f"{what}: host argument {a.name}")
            else:
                for b, w in zip(self.bufs[a.name], a.cols):
                    same(b.read(), w, f"{what}: device argument {a.name}")


def planted(arg, seed):
    """-> (the argument with one non-canonical element, the column, row and component the refusal must name)"""
    rng = np.random.default_rng(seed)
    v, bad = PW[arg.field], bad_values(arg.field)
    cols = [w.copy() for w in arg.cols]
    comp = int(rng.integers(3)) if arg.field == FQ3 else 0
    value = bad[int(rng.integers(len(bad)))]
    if arg.kind == "dev":
        c = len(cols) - 1
        r = int(rng.integers(cols[c].size // v))
        plant(arg.field, cols[c], r, value, comp)
        if c:
            plant(arg.field, cols[c], cols[c].size // v - 1, value, comp)         # a later one in the same column: not the one named
        where = (c, r)
    else:
        e = int(rng.integers(cols[0].size // v))
        plant(arg.field, cols[0], e, value, comp)
        where = (e % arg.ncols, e // arg.ncols) if arg.kind == "mat" else (0, e * arg.row_scale)
    return arg._replace(cols=cols), where + (comp if arg.field == FQ3 else None,)


@pytest.fixture
def checked_planner(request):
    pl = backends.planner(request.param)
    yield pl
    pl.checked(False)


@pytest.mark.parametrize("checked_planner", KINDS, indirect=True)
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_checked_mode(checked_planner, case):
    pl = checked_planner
    L = pl.lib
    args, outs, fn = case.make(pl)
    # clean input: the same words checked and unchecked, bit for bit; nothing but the outputs is written
    pl.checked(False)
    off = Run(pl, case, args, outs)
    assert off.call(fn) == MS_OK, L.ms_last_error().decode()
    pl.checked(True)
    assert pl.is_checked
    on = Run(pl, case, args, outs)
    assert on.call(fn) == MS_OK, L.ms_last_error().decode()
    inplace = not outs
    for a, b, g in zip(off.read_outs(), on.read_outs(), outs):
        same(b, a, "checked against unchecked")
        assert not np.array_equal(a, g), "the call wrote its output"
    if inplace:
        for name in off.bufs:
            for a, b in zip(off.bufs[name], on.bufs[name]):
                same(b.read(), a.read(), "checked against unchecked, in place")
    else:
        on.inputs_unchanged("clean, checked")
    # one planted element per argument, host constants included
    for k, arg in enumerate(args):
        bad_arg, (col, row, comp) = planted(arg, 17 * k + CASES.index(case))
        these = [bad_arg if a is arg else a for a in args]
        pl.checked(True)
        run = Run(pl, case, these, outs)
        rc = run.call(fn)
        msg = L.ms_last_error().decode()
        assert rc == MS_ERR_INVALID, (arg.name, rc, msg)
        assert "canonical" in msg and arg.name in msg and any(e in msg for e in case.entries), (arg.name, msg)
        m = re.search(r"column (\d+), row (\d+)(?:, component (\d+))?", msg)
        assert m and (int(m.group(1)), int(m.group(2))) == (col, row), (arg.name, (col, row, comp), msg)
        assert (int(m.group(3)) if m.group(3) else None) == comp, (arg.name, comp, msg)
        for got, guard in zip(run.read_outs(), outs):
            same(got, guard, f"{arg.name}: an output of the refused call")
        run.inputs_unchanged(f"{arg.name}: refused")
        # the same call unchecked is not refused by this mode: it returns what it returned before the mode existed
        pl.checked(False)
        rc = Run(pl, case, these, outs).call(fn)
        assert rc == MS_OK or "checked mode" not in L.ms_last_error().decode(), (arg.name, rc)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5  classification of the header's entry points
# ---------------------------------------------------------------------------------------------------------------------------------
CHECKS, MOVES, NOFIELD = "checks", "moves words", "no field data"
CLASSES = {
    **{n: CHECKS for n in (
        "ms_ntt_plan_create", "ms_ntt_encode", "ms_ntt_execute", "ms_ntt_enqueue", "ms_ntt_enqueue_to", "ms_lde", "ms_evaluate", "ms_binary",
        "ms_binary_const", "ms_mul_pow", "ms_unary", "ms_convert", "ms_fill", "ms_sum_columns", "ms_sha256_rows", "ms_sha256_rows_row_major",
        "ms_blake2s_rows", "ms_blake2s_rows_row_major", "ms_rpo256_rows", "ms_rpo256_rows_row_major", "ms_rpo256_rows_field", "ms_rpo256_merkle",
        "ms_eval_program", "ms_eval_program_ex", "ms_validate_constraints", "ms_scan_affine", "ms_fri_fold", "ms_fri_fold_rows", "ms_horner_eval",
        "ms_deep_rows", "ms_deep_compose")},
    **{n: MOVES for n in (
        "ms_copy", "ms_upload", "ms_download", "ms_bit_reverse", "ms_deinterleave", "ms_gather_rows", "ms_gather_digests", "ms_gather_digests_multi",
        "ms_sha256_merkle", "ms_blake2s_merkle", "ms_sha256_pow_grind", "ms_blake2s_pow_grind", "ms_cols_to_rows_alltoall", "ms_allgather_digests",
        "ms_p2p_batch")},
    **{n: NOFIELD for n in (
        "ms_ctx_create", "ms_ctx_destroy", "ms_sync", "ms_ctx_stream", "ms_last_error", "ms_field_bytes", "ms_profile_enable", "ms_profile_read",
        "ms_alloc", "ms_free", "ms_ntt_plan_destroy", "ms_eval_jit_check", "ms_eval_jit_stats", "ms_merkle_view_ids", "ms_comm_unique_id",
        "ms_comm_init", "ms_comm_destroy", "ms_comm_rank", "ms_cols_to_rows_schedule", "ms_check_canonical", "ms_check_canonical_host",
        "ms_ctx_set_checked", "ms_ctx_get_checked")},
}


def test_every_entry_point_is_classified():
    src = open(os.path.join(ROOT, "include", "ministark_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ms_[a-z0-9_]+)\s*\(", src))
    assert declared == set(CLASSES), declared ^ set(CLASSES)
    reached = {e for c in CASES for e in c.entries}
    checks = {n for n, k in CLASSES.items() if k == CHECKS}
    assert reached == checks, reached ^ checks
    for f, names in ((FQ3, checks - {"ms_rpo256_rows", "ms_rpo256_rows_row_major", "ms_rpo256_merkle"}), (F252, checks - {n for n in checks if "rpo256" in n})):
        assert {e for c in CASES if c.field == f for e in c.entries} == names            # per field the family takes
    text = open(os.path.join(ROOT, "include", "ministark_hip.h")).read()
    doc = text[text.index("---- checked mode"):text.index("typedef struct ms_canon_report")]
    for n in ("ms_copy", "ms_upload", "ms_download", "ms_bit_reverse", "ms_deinterleave", "ms_gather_rows", "ms_gather_digests", "BLOCKS"):
        assert n in doc, n


# ---------------------------------------------------------------------------------------------------------------------------------
# 6  default and environment
# ---------------------------------------------------------------------------------------------------------------------------------
def test_default_and_environment():
    pl = backends.planner("emu")
    fresh = Planner(0, pl.lib)
    assert fresh.is_checked is False
    fresh.close()
    code = ("import sys, ctypes; sys.path.insert(0, %r); from ministark_amd import _lib, api; "
            "pl = api.Planner(0, _lib.Lib(%r)); print('checked', int(pl.is_checked))" % (ROOT, pl.lib.path))
    for value, want in (("1", 1), ("0", 0), (None, 0), ("", 0)):
        env = {k: v for k, v in os.environ.items() if k != "MS_CHECK_CANONICAL"}
        if value is not None:
            env["MS_CHECK_CANONICAL"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and f"checked {want}" in out.stdout, (value, out.stdout, out.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------------------------
# 7  the Python mirror
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("checked_planner", KINDS, indirect=True)
def test_python_mirror(checked_planner):
    pl = checked_planner
    cols = [clean_words(FQ3, 512, c).reshape(-1, 3) for c in range(3)]
    m = Matrix.from_numpy(pl, cols, FQ3)
    rep = m.check_canonical()
    assert rep and rep.count == 0
    cols[1][300, 2] = P
    cols[2][7, 0] = M64
    m = Matrix.from_numpy(pl, cols, FQ3)
    rep = m.check_canonical()
    assert not rep and (rep.count, rep.first_col, rep.first_row, rep.first_word) == (2, 1, 300, 2)
    assert as_tuple(api.check_canonical(pl, m.columns[2:])) == (1, 0, 7, 0)
    assert api.check_canonical(pl, []).count == 0
    before = [c.copy() for c in m.to_numpy()]
    assert pl.checked() is pl and pl.is_checked
    with pytest.raises(_lib.MsError, match=r"canonical.*column 1, row 300, component 2") as e:
        m.hash_rows()
    assert e.value.code == MS_ERR_INVALID
    with pytest.raises(_lib.MsError, match="d_columns.*canonical"):
        m.into_polynomials(api.Radix2EvaluationDomain.new(512))
    pl.sync()
    for a, b in zip(m.to_numpy(), before):
        assert np.array_equal(a, b)
    pl.checked(False)
    m.hash_rows()
    pl.sync()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8  rate
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scan_rate_against_negation():
    """8 Fp columns of 2^24 elements: the scan (1.07 GB read, nothing written) against eight ms_unary(MS_NEG) calls into disjoint
    destinations over the same buffers (twice the bytes).  Kernel time from the library's per-launch events, median of 5, alternating."""
    pl = backends.planner("hip")
    n, ncols = 1 << 24, 8
    rng = np.random.default_rng(8)
    src = [api.GpuVec.from_numpy(pl, rng.integers(0, P, size=n, dtype=np.uint64), FP) for _ in range(ncols)]
    dst = [api.GpuVec(pl, n, FP) for _ in range(ncols)]
    ptrs = [v.ptr for v in src]

    def neg():
        for s, d in zip(src, dst):
            assert pl.lib.ms_unary(pl.handle, 0, FP, n, d.ptr, s.ptr, 0) == MS_OK

    def timed(fn, name):
        pl.profile(True)
        fn()
        t = pl.profile_read()[name]["total_us"]
        pl.profile(False)
        return t
    for _ in range(2):
        assert scan(pl, FP, n, ptrs).count == 0
        neg()
    pl.sync()
    ts, tn = [], []
    for _ in range(5):
        ts.append(timed(lambda: scan(pl, FP, n, ptrs), "canon_scan"))
        tn.append(timed(neg, "stage_neg"))
    scan_us, neg_us = float(np.median(ts)), float(np.median(tn))
    print(f"canon_scan {scan_us:.1f} us ({8.0 * n * ncols / scan_us / 1e6:.2f} TB/s read), 8 x stage_neg {neg_us:.1f} us ({16.0 * n * ncols / neg_us / 1e6:.2f} TB/s moved)")
    assert scan_us <= neg_us, (scan_us, neg_us)
