"""ms_sort_rows and ms_permute_columns (include/ministark_hip_sort.h) against the loop on Python integers (tests/sort_ref.py): every word of
the permutation, of the permuted columns and of the report.

    T = 2048   rows a workgroup handles in a pass (mssort::TILE: 256 threads, 8 rows each; a wave takes 512 consecutive rows)
    B = 256    workgroups past which the per-digit scan of the tile histograms takes one more round (mssort::SCAN_ROUND)

Lengths 1, 2, 3, T-1, T, T+1, 2T+1 on both backends and B T + 3 on the device only (the simulator takes minutes for it), both fields, 1..4 key
components, the three masks in rotation (and 64 T + 1 and 128 T + 1 rows, where the scan changes its width), no row and one row active; keys that are a shuffle of 0..n-1 (a sort by Montgomery words fails);
keys that vary in one byte and in two adjacent bytes, at every byte (odd and even numbers of executed passes: the buffer parity); few
distinct keys at n = 4097 (stability: the expected permutation is the reference's, not merely a sorted one -- on the device this is what
meets a rank taken in arrival order); all keys equal, sorted, reversed, 0 and p - 1; the gather with repeats, shorter and longer outputs
and entries past the source; five equal runs; and the refusals, after which the sentinel-filled outputs are unchanged."""
import ctypes
import functools

import numpy as np
import pytest

from tests import backends
from tests.ext_ref import PAIRS
from tests.sort_ref import permuted, reference
from ministark_amd import DeviceIndex, GpuVec, Matrix, SortKey, extension, permute_columns, sort_rows
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, STARK252_FP as F252F
from ministark_amd._lib import MsError, SortReportRecord

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = {"fp": PAIRS["fp_fp"], "fp252": PAIRS["fp252_fp252"]}
T, B = 2048, 256
LENGTHS = [1, 2, 3, T - 1, T, T + 1, 2 * T + 1]
INVALID, UNSUPPORTED = -1, -2
SENTINEL = 0xA5A5A5A5A5A5A5A5
MASKS = [None, "nonzero", "zero"]


def upload(pl, pair, base):
    return Matrix([GpuVec.from_numpy(pl, pair.base_words(c), pair.base_field) for c in base])


def run(kind, fname, base, key, n=None, runs=1):
    """sort on the backend, compare permutation and report with the reference; -> (perm, report of the reference)"""
    pl, pair = backends.planner(kind), FIELDS[fname]
    want, rep = reference(base, key, 8 * pair.bf.nlimbs, n)
    d_base = upload(pl, pair, base)
    for _ in range(runs):
        perm, report = sort_rows(pl, d_base, key, n=n)
        got = perm.to_numpy()
        bad = np.nonzero(got != np.array(want, dtype=np.uint32))[0]
        assert bad.size == 0, (fname, key.cols, key.mask, f"{bad.size} entries differ, the first at {int(bad[0])}: {int(got[bad[0]])} for {want[int(bad[0])]}")
        assert (report.active, report.varying_bytes) == (rep["active"], rep["varying_bytes"]), (fname, key.cols, repr(report), rep)
    for c, v in zip(d_base.columns, base):                                      # the inputs are only read
        assert np.array_equal(c.to_numpy(), pair.base_words(v))
    return want, rep


@functools.lru_cache(maxsize=None)
def random_base(fname, n, nkeys, small, seed=0):
    """nkeys key columns and one mask column.  small: the leading components are drawn from few values, so the later ones break ties, and
    the last one from the whole field at n = T + 1 with one component, from 24 bits otherwise (the simulator's time goes with the
    passes; keys that vary in every byte are also in the one-byte and the extreme-keys tests)."""
    pair = FIELDS[fname]
    rng = np.random.default_rng([n, nkeys, seed, pair.bf.nlimbs])
    cols = []
    for k in range(nkeys):
        if small and k < nkeys - 1:
            cols.append([int(v) for v in rng.integers(0, 3, size=n)])
        elif small and not (nkeys == 1 and n == T + 1):
            cols.append([int(v) for v in rng.integers(0, 1 << 24, size=n)])
        else:
            cols.append([int.from_bytes(rng.bytes(40), "little") % pair.bf.p for _ in range(n)])
    cols.append([int(v) if k else 0 for v, k in zip(rng.integers(1, 1 << 62, size=n), rng.integers(0, 3, size=n))])
    return cols


def masked_key(nkeys, kind):
    return SortKey(range(nkeys), None if kind is None else (kind, nkeys))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_fields_and_key_widths(kind, fname, n):
    for nkeys in (1, 2, 3, 4):
        run(kind, fname, random_base(fname, n, nkeys, True), masked_key(nkeys, MASKS[(nkeys + n) % 3]))


@pytest.mark.gpu
@pytest.mark.parametrize("fname,nkeys,tiles", [("fp", 2, 64), ("fp252", 1, 128), ("fp", 2, B), ("fp252", 1, B)])
def test_the_scan_at_its_widths_and_past_one_round(fname, nkeys, tiles):
    """The scan of a digit's tile counts runs 64 threads for up to 64 tiles, 128 for up to 128, 256 beyond, and past B tiles it carries into
    a second round: 64 T + 1, 128 T + 1 and B T + 3 rows.  Keys below 2^20: the reference's sort of half a million integers is what takes
    the time here, not the device."""
    n = tiles * T + (3 if tiles == B else 1)
    rng = np.random.default_rng(n)
    base = [[int(v) for v in rng.integers(0, 1 << 20, size=n)] for _ in range(nkeys)] + [[int(v) for v in rng.integers(0, 2, size=n)]]
    run("hip", fname, base, masked_key(nkeys, "nonzero"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_no_row_and_one_row_active(kind, fname):
    for n in (1, 5, T + 1):
        base = random_base(fname, n, 2, True)[:2]
        for hot in (None, 0, n // 2, n - 1):
            for mk in ("nonzero", "zero"):
                flags = [int((i == hot) == (mk == "nonzero")) for i in range(n)]
                want, rep = run(kind, fname, base + [flags], SortKey([0, 1], (mk, 2)))
                assert rep == {"active": int(hot is not None), "varying_bytes": 0}
                assert want == ([] if hot is None else [hot]) + [i for i in range(n) if i != hot]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_the_order_is_that_of_the_canonical_values_not_of_the_montgomery_words(kind, fname):
    n = T + 1
    keys = [int(v) for v in np.random.default_rng(5).permutation(n)]
    want, rep = run(kind, fname, [keys], SortKey([0]))
    assert [keys[i] for i in want] == list(range(n)) and rep["varying_bytes"] == 2
    pair = FIELDS[fname]
    # Goldilocks maps k < 2^32 to k (2^32 - 1) without a wrap, in order; multiples of 2^40 wrap.  Over Fp252 the shuffle itself does.
    spread = keys if fname == "fp252" else [k << 40 for k in keys]
    mont = [pair.bf.to_mont(k) for k in spread]
    assert sorted(range(n), key=lambda i: mont[i]) != want                      # a sort of the words as they lie gives another order
    if spread is not keys:
        assert run(kind, fname, [spread], SortKey([0]))[0] == want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname,limb", [("fp", 0), ("fp252", 0), ("fp252", 1), ("fp252", 2), ("fp252", 3)])
def test_keys_that_vary_in_one_byte_or_in_two_adjacent_ones(kind, fname, limb):
    """n = 257: every byte position of the second of two components (a case per limb; two adjacent bytes may cross into the next limb); the
    first component is constant, so is every other byte"""
    pair, n = FIELDS[fname], 257
    nbytes = 8 * pair.bf.nlimbs
    top = (pair.bf.p >> (8 * (nbytes - 1))) & 0xFF                              # byte 31 of Fp252 stays below the modulus's top byte
    rng = np.random.default_rng(nbytes)
    fixed = int.from_bytes(rng.bytes(nbytes - 2), "little")
    for b in range(8 * limb, 8 * limb + 8):
        for width in (1, 2):
            if b + width > nbytes:
                continue
            keep = fixed & ~(((1 << (8 * width)) - 1) << (8 * b)) & ((1 << (8 * (nbytes - 1))) - 1)
            limit = [256 if b + k < nbytes - 1 else top for k in range(width)]
            digits = [[int(v) for v in rng.integers(0, limit[k], size=n)] for k in range(width)]
            for k in range(width):                                              # both ends of each byte's range occur, so the byte does vary
                digits[k][k], digits[k][n - 1 - k] = 0, limit[k] - 1
            keys = [keep | sum(digits[k][i] << (8 * (b + k)) for k in range(width)) for i in range(n)]
            assert all(v < pair.bf.p for v in keys)
            _, rep = run(kind, fname, [[7] * n, keys], SortKey([0, 1]))
            assert rep["varying_bytes"] == width, (b, width)


@functools.lru_cache(maxsize=None)
def stability_case(fname, which):
    n = 4097
    rng = np.random.default_rng([which, 4097])
    pair = FIELDS[fname]
    if which < 3:                                                               # 1, 2, 3 distinct keys
        pool = [int.from_bytes(rng.bytes(40), "little") % pair.bf.p for _ in range(which + 1)]
        return [[pool[int(k)] for k in rng.integers(0, which + 1, size=n)]], SortKey([0])
    base = [[int(v) for v in rng.integers(0, 2, size=n)] for _ in range(3)] + [[int(v) for v in rng.integers(0, 4, size=n)]]
    return base, SortKey([0, 1, 2, 3])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_rows_of_equal_keys_keep_their_order(kind, fname, which):
    base, key = stability_case(fname, which)
    want, rep = run(kind, fname, base, key)
    ks = [tuple(base[c][i] for c in key.cols) for i in want]
    assert all(ks[j] < ks[j + 1] or (ks[j] == ks[j + 1] and want[j] < want[j + 1]) for j in range(len(want) - 1))


@pytest.mark.gpu
@pytest.mark.parametrize("fname", list(FIELDS))
def test_five_runs_give_one_result(fname):
    for which in range(4):
        base, key = stability_case(fname, which)
        run("hip", fname, base, key, runs=5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_equal_sorted_reversed_and_extreme_keys(kind, fname):
    pair, n = FIELDS[fname], T + 5
    p = pair.bf.p
    mask = [int(i % 3 != 1) for i in range(n)]
    want, rep = run(kind, fname, [[p - 2] * n, mask], SortKey([0], ("nonzero", 1)))
    assert rep["varying_bytes"] == 0 and want[:rep["active"]] == [i for i in range(n) if mask[i]]          # the identity over the active rows
    asc = [i * 257 for i in range(n)]
    want, _ = run(kind, fname, [asc], SortKey([0]))
    assert want == list(range(n))
    want, _ = run(kind, fname, [asc[::-1]], SortKey([0]))
    assert want == list(range(n))[::-1]
    ends = [(0, p - 1, 1, p - 2)[i % 4] for i in range(n)]
    want, rep = run(kind, fname, [ends], SortKey([0]))
    assert [ends[i] for i in want[:4]] == [0] * 4 and want[:2] == [0, 4] and ends[want[-1]] == p - 1 and rep["varying_bytes"] >= 8


@pytest.mark.parametrize("kind", KINDS)
def test_sorting_the_first_rows_only(kind):
    base = random_base("fp", 300, 2, True)
    run(kind, "fp", base, SortKey([0, 1]), n=299)
    run(kind, "fp", base, masked_key(2, "zero"), n=17)


# ---- ms_permute_columns ----------------------------------------------------------------------------------------------------------------
PFIELDS = {"fp": PAIRS["fp_fp"], "fq3": PAIRS["fp_fq3"], "fp252": PAIRS["fp252_fp252"]}


def permute_case(kind, fname, n_src, ncols, index, n_out=None):
    pl, pair = backends.planner(kind), PFIELDS[fname]
    rng = np.random.default_rng([n_src, ncols])
    vals = [pair.random_ext(rng, n_src) for _ in range(min(ncols, 3))]
    vals = [vals[c % len(vals)][c:] + vals[c % len(vals)][:c] for c in range(ncols)]          # 128 columns: rotations of three
    src = [GpuVec.from_numpy(pl, pair.ext_words(v), pair.ext_field) for v in vals]
    d_index = DeviceIndex.from_numpy(pl, np.array(index, dtype=np.uint32))
    out = permute_columns(pl, src, d_index, n_out=n_out)
    used = index if n_out is None else index[:n_out]
    zero = pair.zero
    for c in range(ncols):
        want = pair.ext_words([vals[c][j] if j < n_src else zero for j in used])
        assert np.array_equal(out.columns[c].to_numpy(), want), (fname, n_src, ncols, c)
        assert np.array_equal(src[c].to_numpy(), pair.ext_words(vals[c]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(PFIELDS))
@pytest.mark.parametrize("n", LENGTHS)
def test_permute_lengths_fields_and_column_counts(kind, fname, n):
    rng = np.random.default_rng(n)
    for ncols in (1, 2, 128):
        if ncols == 128 and n > 3 and n != T + 1:
            continue                                                            # the widest table at the small lengths and at one large one
        permute_case(kind, fname, n, ncols, [int(v) for v in rng.permutation(n)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(PFIELDS))
def test_permute_is_a_gather(kind, fname):
    rng = np.random.default_rng(9)
    n = 300
    permute_case(kind, fname, n, 2, [int(v) for v in rng.integers(0, 7, size=n)])                     # repeats, rows left out
    permute_case(kind, fname, n, 2, [int(v) for v in rng.integers(0, n, size=40)])                    # shorter than the source
    permute_case(kind, fname, n, 2, [int(v) for v in rng.integers(0, n, size=2 * T + 1)])             # longer
    permute_case(kind, fname, n, 2, [int(v) for v in rng.integers(0, n, size=500)], n_out=123)        # a head of the index
    beyond = [int(v) for v in rng.integers(0, 2 * n, size=700)]
    beyond[:4] = [n, n - 1, 0xFFFFFFFF, 1 << 31]
    permute_case(kind, fname, n, 3, beyond)                                                           # entries past the source: zero elements


@pytest.mark.parametrize("kind", KINDS)
def test_sort_then_permute_gives_sorted_columns(kind):
    pl, pair = backends.planner(kind), FIELDS["fp"]
    base = random_base("fp", T + 1, 2, True)
    key = masked_key(2, "nonzero")
    want, rep = reference(base, key, 8)
    d_base = upload(pl, pair, base)
    perm, report = sort_rows(pl, d_base, key)
    out = permute_columns(pl, d_base, perm, n_out=None)
    for c in range(3):
        assert np.array_equal(out.columns[c].to_numpy(), pair.base_words(permuted(base[c], want)))
    assert "active=" in repr(report) and len(perm) == T + 1


# ---- refusals and empty cases ----------------------------------------------------------------------------------------------------------
class SortCall:
    """one raw ms_sort_rows whose arguments a test can bend; d_perm and d_report are filled with a sentinel"""

    def __init__(self, kind, fname="fp", n=300):
        self.pl, self.pair = backends.planner(kind), FIELDS[fname]
        self.base = random_base(fname, n, 3, True)                              # columns 0..2, mask column 3
        self.d_base = upload(self.pl, self.pair, self.base)
        self.field, self.n, self.nkeys, self.V = self.pair.base_field, n, 2, self.pair.bf.nlimbs
        self.base_ptrs = [c.ptr for c in self.d_base.columns]
        self.key = SortKey([0, 1], ("nonzero", 3))._record()
        self.perm = GpuVec.from_numpy(self.pl, np.full((n + 1) // 2, SENTINEL, dtype=np.uint64), FP)
        self.report = GpuVec.from_numpy(self.pl, np.full(2, SENTINEL, dtype=np.uint64), FP)
        self.perm_ptr, self.report_ptr, self.null, self.handle = self.perm.ptr, self.report.ptr, (), self.pl.handle

    def __call__(self):
        rec = np.array(self.key, dtype=np.int32)
        VP = ctypes.c_void_p
        return self.pl.lib.ms_sort_rows(self.handle, self.field, self.n, None if "base" in self.null else (VP * max(1, len(self.base_ptrs)))(*self.base_ptrs),
                                        len(self.base_ptrs), self.nkeys, None if "key" in self.null else rec.ctypes.data, self.perm_ptr, self.report_ptr)

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self):
        assert (self.perm.to_numpy() == np.uint64(SENTINEL)).all() and (self.report.to_numpy() == np.uint64(SENTINEL)).all()


@pytest.mark.parametrize("kind", KINDS)
def test_the_bent_sort_call_is_accepted_unbent(kind):
    call = SortCall(kind)
    assert call() == 0, call.error()
    want, rep = reference(call.base, SortKey([0, 1], ("nonzero", 3)), 8)
    assert np.array_equal(call.perm.to_numpy().view(np.uint32)[:call.n], np.array(want, dtype=np.uint32))
    assert [int(v) for v in call.report.to_numpy()] == [rep["active"], rep["varying_bytes"]]


@pytest.mark.parametrize("kind", KINDS)
def test_sort_null_arguments_widths_indices_and_mask_kinds_are_refused(kind):
    nbase = 4
    bends = [lambda c: setattr(c, "handle", None), lambda c: setattr(c, "null", ("base",)), lambda c: setattr(c, "null", ("key",)),
             lambda c: setattr(c, "perm_ptr", None), lambda c: setattr(c, "report_ptr", None),
             lambda c: c.base_ptrs.__setitem__(2, None), lambda c: setattr(c, "field", 7),
             lambda c: setattr(c, "nkeys", 0), lambda c: setattr(c, "nkeys", 5),
             lambda c: c.key.__setitem__(1, nbase), lambda c: c.key.__setitem__(0, -1),                                # a column
             lambda c: c.key.__setitem__(5, nbase), lambda c: c.key.__setitem__(5, -1),                                # the mask column
             lambda c: c.key.__setitem__(4, 3), lambda c: c.key.__setitem__(4, -1)]                                    # the mask kind
    for k, bend in enumerate(bends):
        call = SortCall(kind)
        assert len(call.base_ptrs) == nbase
        bend(call)
        assert call() == INVALID, (k, call.error())
        call.unchanged()
    call = SortCall(kind)                                                       # what is not read is not checked: components past nkeys, an unmasked key's mask column
    call.key[2], call.key[3] = 99, -7
    assert call() == 0, call.error()
    call = SortCall(kind)
    call.key[4], call.key[5] = 0, 99
    assert call() == 0, call.error()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_sort_outputs_that_overlap_are_refused(kind, fname):
    def refused(bend):
        call = SortCall(kind, fname)
        bend(call)
        assert call() == INVALID and "overlap" in call.error(), call.error()
        call.unchanged()
    col = lambda c: 8 * c.V * c.n
    refused(lambda c: setattr(c, "perm_ptr", c.base_ptrs[0]))                   # a key column
    refused(lambda c: setattr(c, "perm_ptr", c.base_ptrs[3]))                   # the mask column
    refused(lambda c: setattr(c, "perm_ptr", c.base_ptrs[1] + col(c) - 4))      # the last bytes of one
    refused(lambda c: setattr(c, "report_ptr", c.base_ptrs[1] + 8))
    refused(lambda c: setattr(c, "report_ptr", c.perm_ptr))                     # each other
    refused(lambda c: setattr(c, "report_ptr", c.perm_ptr + 4 * c.n - 4))
    call = SortCall(kind, fname)                                                # column 2 is named by neither key nor mask: it may take the permutation
    call.perm_ptr = call.base_ptrs[2]
    assert call() == 0, call.error()


@pytest.mark.parametrize("kind", KINDS)
def test_sort_fq3_and_too_many_rows_are_unsupported_and_no_rows_is_fine(kind):
    for bend in (lambda c: setattr(c, "field", FQ3F), lambda c: setattr(c, "n", (1 << 30) + 1)):
        call = SortCall(kind)
        bend(call)
        assert call() == UNSUPPORTED, call.error()
        call.unchanged()
    call = SortCall(kind)
    call.n = 0
    assert call() == 0, call.error()
    assert (call.perm.to_numpy() == np.uint64(SENTINEL)).all() and not call.report.to_numpy().any()       # a zero report and nothing else
    pl = backends.planner(kind)
    perm, report = sort_rows(pl, upload(pl, FIELDS["fp"], [[3, 1, 2]]), SortKey([0]), n=0)
    assert (report.active, report.varying_bytes, len(perm)) == (0, 0, 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_sort_checked_mode_names_column_and_row(kind, fname):
    pl, pair = backends.planner(kind), FIELDS[fname]
    p_words = [(pair.bf.p >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(pair.bf.nlimbs)]         # p itself: the smallest non-canonical value
    V = len(p_words)
    try:
        pl.checked(True)
        for col, row in ((1, 17), (0, 299), (3, 0)):                            # key columns and the mask column
            call = SortCall(kind, fname)
            w = pair.base_words(call.base[col])
            w[V * row:V * (row + 1)] = p_words
            keep = GpuVec.from_numpy(pl, w, pair.base_field)
            call.base_ptrs[col] = keep.ptr
            assert call() == INVALID, call.error()
            msg = call.error()
            assert "canonical" in msg and "ms_sort_rows" in msg and "d_base" in msg and f"column {col}, row {row};" in msg, msg
            call.unchanged()
        call = SortCall(kind, fname)                                            # a column that the call does not name is not scanned
        keep = GpuVec.from_numpy(pl, np.full(V * call.n, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), pair.base_field)
        call.base_ptrs[2] = keep.ptr
        assert call() == 0, call.error()
    finally:
        pl.checked(False)


class PermuteCall:
    """one raw ms_permute_columns; the destinations are filled with a sentinel"""

    def __init__(self, kind, fname="fp", n_src=300, n_out=200, ncols=3):
        self.pl, self.pair = backends.planner(kind), PFIELDS[fname]
        self.V = 3 if fname == "fq3" else self.pair.bf.nlimbs
        self.field, self.n_src, self.n_out, self.ncols = self.pair.ext_field, n_src, n_out, ncols
        rng = np.random.default_rng(n_out)
        self.src = [GpuVec.from_numpy(self.pl, self.pair.ext_words(self.pair.random_ext(rng, n_src)), self.field) for _ in range(ncols)]
        self.dst = [GpuVec.from_numpy(self.pl, np.full(self.V * n_out, SENTINEL, dtype=np.uint64), self.field) for _ in range(ncols)]
        self.index = DeviceIndex.from_numpy(self.pl, rng.integers(0, n_src, size=n_out).astype(np.uint32))
        self.src_ptrs, self.dst_ptrs, self.index_ptr = [c.ptr for c in self.src], [c.ptr for c in self.dst], self.index.ptr
        self.null, self.handle = (), self.pl.handle

    def __call__(self):
        VP = ctypes.c_void_p
        return self.pl.lib.ms_permute_columns(self.handle, self.field, self.n_src, None if "src" in self.null else (VP * len(self.src_ptrs))(*self.src_ptrs),
                                              None if "dst" in self.null else (VP * len(self.dst_ptrs))(*self.dst_ptrs), self.ncols, self.index_ptr, self.n_out)

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self):
        assert all((d.to_numpy() == np.uint64(SENTINEL)).all() for d in self.dst)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(PFIELDS))
def test_permute_refusals(kind, fname):
    call = PermuteCall(kind, fname)
    assert call() == 0, call.error()
    assert not any((d.to_numpy() == np.uint64(SENTINEL)).any() for d in call.dst)
    bends = [lambda c: setattr(c, "handle", None), lambda c: setattr(c, "null", ("src",)), lambda c: setattr(c, "null", ("dst",)),
             lambda c: setattr(c, "index_ptr", None), lambda c: c.src_ptrs.__setitem__(1, None), lambda c: c.dst_ptrs.__setitem__(2, None),
             lambda c: setattr(c, "field", 7), lambda c: setattr(c, "ncols", 0), lambda c: setattr(c, "ncols", 129)]
    for k, bend in enumerate(bends):
        call = PermuteCall(kind, fname)
        if k == 8:
            call.src_ptrs, call.dst_ptrs = call.src_ptrs * 43, call.dst_ptrs * 43
        bend(call)
        assert call() == INVALID, (k, call.error())
        call.unchanged()
    elem = 8 * call.V
    overlaps = [lambda c: c.dst_ptrs.__setitem__(0, c.src_ptrs[0]),                                   # its own source
                lambda c: c.dst_ptrs.__setitem__(1, c.src_ptrs[2] + elem * (c.n_src - 1)),            # the last element of another
                lambda c: c.dst_ptrs.__setitem__(2, c.index_ptr),                                     # the index
                lambda c: c.dst_ptrs.__setitem__(0, c.index_ptr + 4 * c.n_out - 4),
                lambda c: c.dst_ptrs.__setitem__(2, c.dst_ptrs[0]),                                   # another destination
                lambda c: c.dst_ptrs.__setitem__(1, c.dst_ptrs[2] + elem * (c.n_out - 1))]
    for k, bend in enumerate(overlaps):
        call = PermuteCall(kind, fname)
        bend(call)
        assert call() == INVALID and "overlap" in call.error(), (k, call.error())
        call.unchanged()
    call = PermuteCall(kind, fname)                                             # no output rows: accepted, nothing written
    call.n_out = 0
    assert call() == 0, call.error()
    call.unchanged()


def test_python_mirror_argument_checks():
    pl, pair = backends.planner("emu"), FIELDS["fp"]
    d_base = upload(pl, pair, [[1, 2], [2, 1]])
    with pytest.raises(MsError) as err:
        sort_rows(pl, d_base, SortKey([9]))
    assert err.value.code == INVALID and "out of range" in str(err.value)
    for bad in (lambda: SortKey([]), lambda: SortKey([0, 1, 2, 3, 4]), lambda: SortKey([0], mask=("odd", 1)), lambda: sort_rows(pl, d_base, SortKey([0]), n=3),
                lambda: sort_rows(pl, [], SortKey([0]))):
        with pytest.raises(ValueError):
            bad()
    perm, _ = sort_rows(pl, d_base, SortKey([1]))
    assert [int(v) for v in perm.to_numpy()] == [1, 0]
    with pytest.raises(ValueError):
        permute_columns(pl, d_base, perm, n_out=3)
    with pytest.raises(ValueError):
        permute_columns(pl, d_base, perm, out=[GpuVec(pl, 2, FP)])
    with pytest.raises(MsError) as err:
        permute_columns(pl, d_base, perm, out=d_base)
    assert err.value.code == INVALID and "overlap" in str(err.value)
    out = [GpuVec.from_numpy(pl, np.full(3, SENTINEL, dtype=np.uint64), FP) for _ in range(2)]
    got = permute_columns(pl, d_base, perm, out=out)                            # longer destinations: their first n_out elements are filled
    assert got.columns[0] is out[0] and [int(v) for v in out[0].to_numpy()] == [int(v) for v in pair.base_words([2, 1])] + [SENTINEL]
    assert (extension.SORT_MAX_KEYS, extension.PERMUTE_MAX_COLUMNS) == (4, 128) and ctypes.sizeof(SortReportRecord) == 16
    assert F252F in (f.base_field for f in FIELDS.values())
