"""ms_range_multiplicities (include/ministark_hip_range.h) against the loop on Python integers (tests/range_ref.py), and against
ms_lookup_multiplicities on the table column min(j, 2^bits - 1) -- the route it replaces -- word for word: every table size class (32-bit
LDS counters, the largest such table, packed 16-bit counters, the global form) with each counting kernel forced through MS_RANGE_FORM,
both fields, the packed counters' flush (131 072 rows on one bin, and on the two bins of one word), values at and past the table's end,
252-bit values whose low word alone is in range, 64 sets, the three masks, a zero tail past the table -- and the refusals, after which
the sentinel-filled d_m and d_report are unchanged."""
import ctypes
import functools

import numpy as np
import pytest

from tests import backends
from tests.ext_ref import PAIRS
from tests.range_ref import RANGE_REPORT_FIELDS, range_multiplicities as reference
from ministark_amd import GpuVec, LookupMissing, LookupTuple, Matrix, RangeReport, RangeSet, extension, lookup_multiplicities, range_multiplicities
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F
from ministark_amd._lib import LookupReportRecord, MsError

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = {"fp": PAIRS["fp_fp"], "fp252": PAIRS["fp252_fp252"]}
FORMS = [None, "plain", "lds"]
INVALID, UNSUPPORTED = -1, -2
SENTINEL = 0xA5A5A5A5A5A5A5A5


@functools.lru_cache(maxsize=None)
def mont_words(fname, v):
    return tuple(int(w) for w in FIELDS[fname].base_words([v]))


def words(fname, vals):
    return np.array([w for v in vals for w in mont_words(fname, v)], dtype=np.uint64)


def upload(pl, fname, cols):
    return Matrix([GpuVec.from_numpy(pl, words(fname, c), FIELDS[fname].base_field) for c in cols])


def mask_column(rng, n):
    return [int(v) if k else 0 for v, k in zip(rng.integers(1, 1 << 62, size=n), rng.integers(0, 3, size=n))]


def report_dict(report):
    return {k: getattr(report, k) for k in RANGE_REPORT_FIELDS}


def lookups(pair, rng, bits, n, shape):
    """n looked-up values: "uniform" over the table and a few past it, "high" half zero and half uniform, "zero" """
    top = 1 << bits
    if shape == "zero":
        return [0] * n
    vals = [int(v) for v in rng.integers(0, top + max(1, top // 16), size=n)]
    if shape == "high":
        vals = [0 if k else v for v, k in zip(vals, rng.integers(0, 2, size=n))]
    edges = [top - 1, top, pair.bf.p - 1, 0, top + 1, 1 << 32, (1 << 32) + 1, 1 << 63]
    if pair.bf.nlimbs == 4:
        edges += [(1 << 64) + 1, (1 << 128) + (top - 1), (1 << 192) + 2, (1 << 251) + 0]
    for k, e in enumerate(edges[:n]):
        vals[(7 * k + 3) % n] = e
    return vals


def run(kind, fname, base, bits, sets, n_m, what, form=None, monkeypatch=None, in_place=None):
    pl, pair = backends.planner(kind), FIELDS[fname]
    want, rep = reference(base, bits, sets, n_m)
    d = upload(pl, fname, base)
    out = d.columns[in_place] if in_place is not None else GpuVec.from_numpy(pl, np.full(n_m * pair.bf.nlimbs, SENTINEL, dtype=np.uint64), pair.base_field)
    if form is not None:
        monkeypatch.setenv("MS_RANGE_FORM", form)
    m, report = range_multiplicities(pl, d, bits, sets, out=out, n_m=n_m)
    assert m is out and isinstance(report, RangeReport)
    got, exp = m.to_numpy()[:n_m * pair.bf.nlimbs], words(fname, want)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (what, f"{bad.size} words of m differ, the first is word {int(bad[0])}")
    assert report_dict(report) == rep, what
    for k, (c, v) in enumerate(zip(d.columns, base)):                           # the looked-up columns are only read
        assert k == in_place or np.array_equal(c.to_numpy(), words(fname, v)), what
    return want, rep, report


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bits", [1, 8, 14, 15, 16, 17])
def test_every_table_class_in_every_form(kind, fname, form, bits, monkeypatch):
    """three sets, one of each mask kind, of the three value shapes; n is no multiple of a workgroup; n_m is a few rows past the table.
    Forcing `lds` on a table that has no LDS form leaves the global one: the result is the same."""
    pair, n = FIELDS[fname], 2500
    rng = np.random.default_rng([bits, n])
    base = [lookups(pair, rng, bits, n, s) for s in ("uniform", "high", "zero")] + [mask_column(rng, n)]
    sets = [RangeSet(0, ("nonzero", 3)), RangeSet(1), RangeSet(2, ("zero", 3))]
    want, rep, _ = run(kind, fname, base, bits, sets, (1 << bits) + 5, (fname, form, bits), form, monkeypatch)
    assert rep["missing"] > 0 and want[0] > n // 3 and sum(want) + rep["missing"] > n


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("bits", [1, 8, 12])
def test_it_equals_lookup_multiplicities_on_the_iota_table(kind, fname, bits):
    """n_m = n: m and the report equal, word for word, what the hash-table route gives against t[j] = min(j, 2^bits - 1), on the same columns"""
    pl, pair = backends.planner(kind), FIELDS[fname]
    n = (1 << bits) + 37
    rng = np.random.default_rng([bits, 37])
    base = [lookups(pair, rng, bits, n, "uniform"), lookups(pair, rng, bits, n, "high"), mask_column(rng, n), [min(j, (1 << bits) - 1) for j in range(n)]]
    d = upload(pl, fname, base)
    masks = [("nonzero", 2), None]
    m_l, rep_l = lookup_multiplicities(pl, d, LookupTuple([3]), [LookupTuple([c], mk) for c, mk in enumerate(masks)])
    m_r, rep_r = range_multiplicities(pl, d, bits, [RangeSet(c, mk) for c, mk in enumerate(masks)])
    assert len(m_r) == n and np.array_equal(m_r.to_numpy(), m_l.to_numpy())
    a, b = rep_l.buf.to_numpy(), rep_r.buf.to_numpy()
    assert np.array_equal(a[:3], b[:3]) and rep_r.missing == rep_l.missing > 0
    assert (rep_r.first_missing_set, rep_r.first_missing_row) == (rep_l.first_missing_set, rep_l.first_missing_row)
    assert rep_l.duplicate_table_rows == 37 and rep_r.duplicate_table_rows == 0            # the one field that is the table's, not the lookups'
    want, rep = reference(base, bits, [RangeSet(c, mk) for c, mk in enumerate(masks)], n)
    assert np.array_equal(m_r.to_numpy(), words(fname, want)) and report_dict(rep_r) == rep


def fp_mont(a):
    """Montgomery words of values below 2^32 over Goldilocks: x * (2^32 - 1), exact in 64 bits"""
    a = np.asarray(a, dtype=np.uint64)
    return (a << np.uint64(32)) - a


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", FORMS)
def test_the_packed_counters_are_flushed_before_they_wrap(kind, form, monkeypatch):
    """bits = 16, 2^17 rows: every row of set 0 is 40 000 and every row of set 1 is 40 001 -- the two halves of ONE packed word, each
    counted 131 072 times, which 16 bits do not hold.  A missing flush loses counts; a late one carries the low half into the high."""
    pl, n = backends.planner(kind), 1 << 17
    cols = [GpuVec.from_numpy(pl, fp_mont(np.full(n, v)), FP) for v in (40000, 40001)]
    if form is not None:
        monkeypatch.setenv("MS_RANGE_FORM", form)
    m, report = range_multiplicities(pl, cols, 16, [RangeSet(0), RangeSet(1)], n_m=1 << 16)
    want = np.zeros(1 << 16, dtype=np.uint64)
    want[40000] = want[40001] = n
    assert np.array_equal(m.to_numpy(), fp_mont(want)) and report_dict(report) == {k: 0 for k in RANGE_REPORT_FIELDS}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", FORMS)
def test_several_workgroups_share_the_packed_table(kind, form, monkeypatch):
    """bits = 16, 8 sets of 2^17 rows: four workgroups of the LDS form, each flushing more than once; uniform values and a heavy bin"""
    pl, n = backends.planner(kind), 1 << 17
    rng = np.random.default_rng(17)
    v = rng.integers(0, (1 << 16) + 9, size=(2, n), dtype=np.uint64)
    v[1, ::2] = 65535
    cols = [GpuVec.from_numpy(pl, fp_mont(c), FP) for c in v]
    if form is not None:
        monkeypatch.setenv("MS_RANGE_FORM", form)
    sets = [RangeSet(k % 2) for k in range(8)]
    m, report = range_multiplicities(pl, cols, 16, sets, n_m=(1 << 16) + 3)
    cnt = 4 * (np.bincount(v[0].astype(np.int64), minlength=(1 << 16) + 9) + np.bincount(v[1].astype(np.int64), minlength=(1 << 16) + 9))
    want = np.zeros((1 << 16) + 3, dtype=np.uint64)
    want[:1 << 16] = cnt[:1 << 16]
    assert np.array_equal(m.to_numpy(), fp_mont(want))
    first = min((s, int(np.nonzero(v[s] >> np.uint64(16))[0][0])) for s in range(2))
    assert report_dict(report) == {"missing": int(cnt[1 << 16:].sum()), "first_missing_set": first[0], "first_missing_row": first[1], "duplicate_table_rows": 0}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("bits", [8, 16])
def test_every_row_is_zero(kind, fname, bits):
    n = 5000
    want, rep, report = run(kind, fname, [[0] * n, [0] * n], bits, [RangeSet(0), RangeSet(1, ("zero", 0))], 1 << bits, (fname, bits))
    assert want[0] == 2 * n and sum(want) == 2 * n and report and report.check() is report and report.first_missing_values() is None


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("form", ["plain", "lds"])
def test_the_last_table_row_the_first_value_past_it_and_p_minus_one(kind, fname, form, monkeypatch):
    pair = FIELDS[fname]
    for bits in (1, 12, 15, 16):
        top = 1 << bits
        col = [top - 1, top, pair.bf.p - 1, top - 1, 0, top + 1]
        if fname == "fp252":                                                    # the low word is a table row, a higher word is not zero: not in the table
            col += [(1 << 64) + 3, (1 << 128) + (top - 1), (1 << 192), (5 << 192) + 1, (1 << 64) * (top - 1)]
        want, rep, report = run(kind, fname, [col], bits, [RangeSet(0)], top, (fname, bits), form, monkeypatch)
        assert want[top - 1] == 2 and want[0] == 1 and sum(want) == 3 and rep["missing"] == len(col) - 3 and rep["first_missing_row"] == 1
        with pytest.raises(LookupMissing) as err:
            report.check()
        assert (err.value.set, err.value.row, err.value.values, err.value.missing) == (0, 1, [top], len(col) - 3)
        assert "set 0, row 1" in str(err.value) and f"value {top} " in str(err.value) and f"2^{bits}" in str(err.value)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_sixty_four_sets_with_masks(kind, fname):
    pair, n, bits = FIELDS[fname], 257, 9
    rng = np.random.default_rng(64)
    base = [lookups(pair, rng, bits, n, ("uniform", "high")[c % 2]) for c in range(4)] + [mask_column(rng, n), mask_column(rng, n)]
    sets = [RangeSet(k % 4, [None, ("nonzero", 4 + k % 2), ("zero", 4 + (k + 1) % 2)][k % 3]) for k in range(64)]
    want, rep, _ = run(kind, fname, base, bits, sets, 1 << bits, fname)
    assert rep["missing"] > 64 and (rep["first_missing_set"], rep["first_missing_row"]) != (0, 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_m_may_be_a_column_of_the_trace_that_nothing_names(kind, fname):
    pair, n, bits = FIELDS[fname], 700, 9
    rng = np.random.default_rng(700)
    base = [lookups(pair, rng, bits, n, "uniform"), mask_column(rng, n), [SENTINEL % pair.bf.p] * n]
    run(kind, fname, base, bits, [RangeSet(0, ("nonzero", 1))], n, fname, in_place=2)          # n_m = n > 2^bits: the tail is zero


@pytest.mark.gpu
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("bits", [8, 16, 17])
def test_the_result_is_the_same_on_every_run(fname, bits):
    """2^17 rows, three sets: many workgroups add to the same counters.  Three times in one process: the same words, and the reference's."""
    pl, pair, n = backends.planner("hip"), FIELDS[fname], 1 << 17
    rng = np.random.default_rng([bits, 17])
    v = rng.integers(0, (1 << bits) + 3, size=(2, n), dtype=np.uint64)
    v[1, ::2] = 0
    cnt = np.bincount(v[0].astype(np.int64), minlength=(1 << bits) + 3) + 2 * np.bincount(v[1].astype(np.int64), minlength=(1 << bits) + 3)
    if fname == "fp":
        cols = [GpuVec.from_numpy(pl, fp_mont(c), FP) for c in v]
        want = fp_mont(cnt[:1 << bits])
    else:
        cols = [GpuVec.from_numpy(pl, words(fname, [int(x) for x in c]), pair.base_field) for c in v]
        want = words(fname, [int(x) for x in cnt[:1 << bits]])
    runs = []
    for _ in range(3):
        m, report = range_multiplicities(pl, cols, bits, [RangeSet(0), RangeSet(1), RangeSet(1)], n_m=1 << bits)
        runs.append((m.to_numpy(), report.buf.to_numpy()))
        assert report.missing == int(cnt[1 << bits:].sum())
    assert np.array_equal(runs[0][0], want)
    assert all(np.array_equal(runs[0][0], r[0]) and np.array_equal(runs[0][1], r[1]) for r in runs[1:])


# ---- refusals and empty cases --------------------------------------------------------------------------------------------------------
class Call:
    """one raw call whose arguments a test can bend: columns 0, 1 looked up, 2, 3 masks, 4 spare; d_m and d_report hold a sentinel"""

    def __init__(self, kind, fname="fp", n=300, bits=7):
        self.pl, self.pair, self.fname = backends.planner(kind), FIELDS[fname], fname
        rng = np.random.default_rng(n)
        self.base = [lookups(self.pair, rng, bits, n, "uniform"), lookups(self.pair, rng, bits, n, "high"), mask_column(rng, n), mask_column(rng, n), [1] * n]
        self.sets = [[0, 1, 2, 0], [1, 2, 3, 0]]
        self.V = self.pair.bf.nlimbs
        self.cols = [GpuVec.from_numpy(self.pl, words(fname, c), self.pair.base_field) for c in self.base]
        self.m = GpuVec.from_numpy(self.pl, np.full(n * self.V, SENTINEL, dtype=np.uint64), self.pair.base_field)
        self.report = GpuVec.from_numpy(self.pl, np.full(4, SENTINEL, dtype=np.uint64), FP)
        self.field, self.n, self.n_m, self.bits, self.nsets, self.nbase = self.pair.base_field, n, n, bits, 2, 5
        self.ptrs, self.m_ptr, self.report_ptr, self.null, self.handle = [c.ptr for c in self.cols], self.m.ptr, self.report.ptr, (), self.pl.handle

    def __call__(self):
        rec = np.array(self.sets, dtype=np.int32).reshape(-1, 4)
        arr = None if "base" in self.null else (ctypes.c_void_p * len(self.ptrs))(*self.ptrs)
        return self.pl.lib.ms_range_multiplicities(self.handle, self.field, self.n, arr, self.nbase, self.bits, None if "sets" in self.null else rec.ctypes.data,
                                                   self.nsets, self.n_m, self.m_ptr, self.report_ptr)

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self):
        assert (self.m.to_numpy() == np.uint64(SENTINEL)).all() and (self.report.to_numpy() == np.uint64(SENTINEL)).all()

    def record(self):
        rec = LookupReportRecord.from_buffer_copy(self.report.to_numpy().tobytes())
        return {k: int(getattr(rec, k)) for k in RANGE_REPORT_FIELDS}

    def expected(self, n=None):
        mk = lambda r: None if r[1] == 0 else (("nonzero", "zero")[r[1] - 1], r[2])
        return reference(self.base, self.bits, [RangeSet(r[0], mk(r)) for r in self.sets[:self.nsets]], self.n_m, self.n if n is None else n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_the_bent_call_is_accepted_unbent(kind, fname):
    call = Call(kind, fname)
    assert call() == 0, call.error()
    want, rep = call.expected()
    assert np.array_equal(call.m.to_numpy(), words(fname, want)) and call.record() == rep and rep["missing"] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_null_arguments_limits_indices_and_mask_kinds_are_refused(kind, monkeypatch):
    S = lambda k, w, v: (lambda c: c.sets[k].__setitem__(w, v))
    bends = [(lambda c: setattr(c, "handle", None), "null"), (lambda c: setattr(c, "null", ("base",)), "null"), (lambda c: setattr(c, "null", ("sets",)), "null"),
             (lambda c: setattr(c, "m_ptr", None), "null"), (lambda c: setattr(c, "report_ptr", None), "null"), (lambda c: c.ptrs.__setitem__(4, None), "null base column 4"),
             (lambda c: setattr(c, "field", 7), ""), (lambda c: setattr(c, "bits", 0), "bits"), (lambda c: setattr(c, "bits", 25), "bits"),
             (lambda c: setattr(c, "n_m", 127), "fewer than the 2^7 rows"), (lambda c: setattr(c, "bits", 9), "fewer than the 2^9 rows"),
             (S(0, 0, 5), "out of range"), (S(1, 0, -1), "out of range"), (S(0, 2, 5), "mask"), (S(1, 2, -1), "mask"), (S(0, 1, 3), "mask kind"), (S(1, 1, -1), "mask kind")]
    for k, (bend, text) in enumerate(bends):
        call = Call(kind)
        bend(call)
        assert call() == INVALID and text in call.error(), (k, call.error())
        call.unchanged()
    call = Call(kind)
    call.sets[1][0] = 5
    assert call() == INVALID and "set 1" in call.error() and "out of range" in call.error(), call.error()
    monkeypatch.setenv("MS_RANGE_FORM", "fast")
    call = Call(kind)
    assert call() == INVALID and "MS_RANGE_FORM" in call.error(), call.error()
    call.unchanged()
    monkeypatch.delenv("MS_RANGE_FORM")
    call = Call(kind)                                                           # what is not read is not checked: an unmasked set's mask column
    call.sets[0][1:3] = [0, 99]
    assert call() == 0, call.error()
    call = Call(kind)                                                           # n_m = 2^bits exactly, shorter than the columns
    call.n_m = 128
    assert call() == 0, call.error()
    want, rep = call.expected()
    got = call.m.to_numpy()
    assert np.array_equal(got[:128], words("fp", want)) and (got[128:] == np.uint64(SENTINEL)).all() and call.record() == rep


@pytest.mark.parametrize("kind", KINDS)
def test_what_is_too_large_and_fq3_are_unsupported(kind):
    """64 sets of 2^26 rows are 2^32 counted rows: refused from the arguments alone -- the columns here hold 300"""
    for bend in (lambda c: (setattr(c, "nsets", 65), setattr(c, "sets", c.sets[:1] * 65)), lambda c: setattr(c, "field", FQ3F),
                 lambda c: (setattr(c, "nsets", 64), setattr(c, "sets", c.sets[:1] * 64), setattr(c, "n", 1 << 26)),
                 lambda c: (setattr(c, "nsets", 1), setattr(c, "n", 1 << 32)), lambda c: setattr(c, "n", (1 << 32) + 1)):
        call = Call(kind)
        bend(call)
        assert call() == UNSUPPORTED, call.error()
        call.unchanged()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_overlapping_outputs_are_refused(kind, fname):
    def refused(bend):
        call = Call(kind, fname)
        bend(call)
        assert call() == INVALID and "overlap" in call.error(), call.error()
        call.unchanged()
    col = lambda c: 8 * c.V * c.n
    refused(lambda c: setattr(c, "m_ptr", c.ptrs[0]))                            # a looked-up column
    refused(lambda c: setattr(c, "m_ptr", c.ptrs[3]))                            # a mask column
    refused(lambda c: setattr(c, "m_ptr", c.ptrs[1] + col(c) - 8))               # the last word of one
    refused(lambda c: setattr(c, "report_ptr", c.ptrs[2] + 8))
    refused(lambda c: setattr(c, "report_ptr", c.ptrs[0] + col(c) - 8))
    refused(lambda c: setattr(c, "report_ptr", c.m_ptr))                         # each other
    refused(lambda c: setattr(c, "report_ptr", c.m_ptr + col(c) - 8))
    call = Call(kind, fname)                                                    # the spare column may take m
    call.m_ptr = call.ptrs[4]
    assert call() == 0, call.error()
    want, rep = call.expected()
    assert np.array_equal(call.cols[4].to_numpy(), words(fname, want)) and call.record() == rep


@pytest.mark.parametrize("kind", KINDS)
def test_no_rows_and_no_sets(kind):
    for bend in (lambda c: setattr(c, "n", 0), lambda c: (setattr(c, "nsets", 0), setattr(c, "null", ("sets",))), lambda c: (setattr(c, "n", 0), setattr(c, "nsets", 0))):
        call = Call(kind)
        bend(call)
        assert call() == 0, call.error()
        assert (call.m.to_numpy() == 0).all() and call.record() == {k: 0 for k in RANGE_REPORT_FIELDS}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_checked_mode_names_column_and_row(kind, fname):
    pl, pair = backends.planner(kind), FIELDS[fname]
    p_words = [(pair.bf.p >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(pair.bf.nlimbs)]          # p itself: the smallest non-canonical value
    V = len(p_words)
    try:
        pl.checked(True)
        for col, row in ((0, 17), (1, 299), (2, 0), (3, 150)):
            call = Call(kind, fname)
            w = words(fname, call.base[col])
            w[V * row:V * (row + 1)] = p_words
            keep = GpuVec.from_numpy(pl, w, pair.base_field)
            call.ptrs[col] = keep.ptr
            assert call() == INVALID, call.error()
            msg = call.error()
            assert "canonical" in msg and "ms_range_multiplicities" in msg and "d_base" in msg and f"column {col}, row {row};" in msg, msg
            call.unchanged()
        call = Call(kind, fname)                                                # a column that no set names is not scanned, and may take m
        bad = GpuVec.from_numpy(pl, np.full(call.n * V, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), pair.base_field)
        call.ptrs[4] = call.m_ptr = bad.ptr
        assert call() == 0, call.error()
        want, rep = call.expected()
        assert np.array_equal(bad.to_numpy(), words(fname, want)) and call.record() == rep
    finally:
        pl.checked(False)


def test_python_mirror_argument_checks():
    pl = backends.planner("emu")
    d = upload(pl, "fp", [[3, 0, 3, 4, 1], [0, 0, 1, 0, 0]])
    m, report = range_multiplicities(pl, d, 2, [RangeSet(0)])
    assert len(m) == 5 and list(m.to_numpy()) == list(words("fp", [1, 1, 0, 2, 0])) and not report
    assert (report.missing, report.first_missing_set, report.first_missing_row, report.first_missing_values()) == (1, 0, 3, [4])
    m, report = range_multiplicities(pl, d, 2, [RangeSet(0, ("zero", 1))], n_m=4)
    assert len(m) == 4 and list(m.to_numpy()) == list(words("fp", [1, 1, 0, 1])) and report.missing == 1
    m, report = range_multiplicities(pl, d, 2, [])
    assert list(m.to_numpy()) == [0] * 5 and report.check() is report
    with pytest.raises(MsError) as err:
        range_multiplicities(pl, d, 2, [RangeSet(2)])
    assert err.value.code == INVALID and "out of range" in str(err.value)
    with pytest.raises(MsError) as err:
        range_multiplicities(pl, d, 2, [RangeSet(0)], out=d.columns[0])
    assert err.value.code == INVALID and "overlap" in str(err.value)
    for bad in (lambda: range_multiplicities(pl, d, 3, [RangeSet(0)]), lambda: range_multiplicities(pl, d, 0, [RangeSet(0)]), lambda: range_multiplicities(pl, d, 25, [RangeSet(0)]),
                lambda: range_multiplicities(pl, d, 2, [RangeSet(0)] * 65), lambda: range_multiplicities(pl, d, 2, [RangeSet(0)], n_m=3),
                lambda: range_multiplicities(pl, d, 2, [RangeSet(0)], out=GpuVec(pl, 4, FP), n_m=5), lambda: RangeSet(0, ("odd", 1))):
        with pytest.raises(ValueError):
            bad()
    assert (extension.RANGE_MAX_SETS, extension.RANGE_MAX_TABLE_BITS) == (64, 24)
