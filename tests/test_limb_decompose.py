"""ms_limb_decompose (include/ministark_hip_range.h) against the loop on Python integers (tests/range_ref.py), every limb column and the
report word for word: limb widths that divide 64 and widths that put limbs across word boundaries, both fields, lengths round the
workgroup size, the edge values of every shape (0, 1, the largest value that fits, the smallest that does not, p - 1, top-word-only
values), the three masks, 64 specs in one call, overflow in several specs, recomposition -- and the refusals, after which the
sentinel-filled destinations and report are unchanged.  What only the device can show -- a lane's second row past the grid cap, and two
runs equal in every word -- is the `hip` half of every case and the two GPU-only tests."""
import ctypes
import functools

import numpy as np
import pytest

from tests import backends
from tests.ext_ref import PAIRS
from tests.range_ref import LIMB_REPORT_FIELDS, limb_decompose as reference
from ministark_amd import GpuVec, LimbReport, LimbSpec, LookupMissing, Matrix, extension, limb_decompose
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F
from ministark_amd._lib import LimbReportRecord, MsError

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = {"fp": PAIRS["fp_fp"], "fp252": PAIRS["fp252_fp252"]}
SHAPES = {"fp": [(1, 64), (16, 4), (32, 2), (7, 9), (12, 5), (20, 3), (24, 2)], "fp252": [(32, 8), (28, 9), (1, 252), (16, 16)]}
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1025]
INVALID, UNSUPPORTED = -1, -2
SENTINEL = 0xA5A5A5A5A5A5A5A5


@functools.lru_cache(maxsize=None)
def mont_words(fname, v):
    return tuple(int(w) for w in FIELDS[fname].base_words([v]))


def words(fname, vals):
    return np.array([w for v in vals for w in mont_words(fname, v)], dtype=np.uint64)


def edge_values(pair, bits, nlimbs):
    """what a decomposition can get wrong at its ends, all below p"""
    p, total = pair.bf.p, bits * nlimbs
    vals = [0, 1, (1 << total) - 1, 1 << total, p - 1, (1 << bits) - 1, 1 << bits, (1 << total) + 1, p - 2]
    if pair.bf.nlimbs == 4:
        vals += [1 << 192, 5 << 192, (p >> 192) << 192, 1 << 64, 1 << 128, (1 << 64) - 1, (1 << 128) - 1, (1 << 251)]
    else:
        vals += [1 << 32, (1 << 32) - 1, 1 << 63, 0xFFFFFFFF00000000]
    return [v for v in vals if v < p]


def values(pair, rng, bits, nlimbs, n):
    """n values: the edges first, then values that fit and values of the whole field, in turn"""
    total = bits * nlimbs
    out = edge_values(pair, bits, nlimbs)[:n]
    while len(out) < n:
        r = int.from_bytes(rng.bytes(40), "little")
        out.append(r % min(pair.bf.p, 1 << total) if len(out) % 3 else r % pair.bf.p)
    return out


def mask_column(rng, n):
    return [int(v) if k else 0 for v, k in zip(rng.integers(1, 1 << 62, size=n), rng.integers(0, 3, size=n))]


def upload(pl, fname, cols):
    return Matrix([GpuVec.from_numpy(pl, words(fname, c), FIELDS[fname].base_field) for c in cols])


def report_dict(report):
    return {k: getattr(report, k) for k in LIMB_REPORT_FIELDS}


def run(kind, fname, base, specs, what, fill=None):
    """upload `base` (destination columns hold `fill` words when given: they may hold anything), decompose, compare every column and the report"""
    pl, pair = backends.planner(kind), FIELDS[fname]
    want, rep = reference(base, specs)
    d = upload(pl, fname, base)
    if fill is not None:
        for sp in specs:
            for j in range(sp.nlimbs):
                d.columns[sp.dst0 + j] = GpuVec.from_numpy(pl, np.full(len(base[0]) * pair.bf.nlimbs, fill, dtype=np.uint64), pair.base_field)
    report = limb_decompose(pl, d, specs)
    assert isinstance(report, LimbReport)
    for c, (col, w) in enumerate(zip(d.columns, want)):
        got, exp = col.to_numpy(), words(fname, w)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (what, f"column {c}: {bad.size} words differ, the first is word {int(bad[0])}")
    assert report_dict(report) == rep, what
    return want, rep, report


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("n", LENGTHS)
def test_every_shape_at_every_length(kind, fname, n):
    """one spec per call, unmasked and masked in turn; the destinations hold all ones before the call.  Recomposition: the limbs of every
    row that does not overflow sum back to the source."""
    pair = FIELDS[fname]
    for k, (bits, nlimbs) in enumerate(SHAPES[fname]):
        rng = np.random.default_rng([n, bits, nlimbs])
        mask = [None, ("nonzero", 1), ("zero", 1)][(k + n) % 3]
        base = [values(pair, rng, bits, nlimbs, n), mask_column(rng, n)] + [[0] * n for _ in range(nlimbs)]
        spec = LimbSpec(0, 2, nlimbs, bits, mask)
        want, rep, _ = run(kind, fname, base, [spec], (fname, n, bits, nlimbs, mask), fill=0xFFFFFFFFFFFFFFFF)
        if n >= 9 and mask is None:
            assert rep["overflow"] > 0 or bits * nlimbs >= pair.bf.p.bit_length()
            assert rep["active"] == n
        for i in range(n):
            re = sum(want[2 + j][i] << (j * bits) for j in range(nlimbs))
            v = base[0][i]
            if mask is not None and (base[1][i] != 0) != (mask[0] == "nonzero"):
                assert re == 0
            else:
                assert re == v % (1 << (bits * nlimbs)) and (re == v) == (v >> (bits * nlimbs) == 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_sixty_four_specs_in_one_call(kind, fname):
    """64 specs over 4 source columns and 2 mask columns, every mask kind, shapes in turn: 64 disjoint destination ranges"""
    pair, n = FIELDS[fname], 257
    rng = np.random.default_rng(64)
    shapes = SHAPES[fname]
    small = [(b, min(l, 6)) for b, l in shapes]                                # keep the table narrow: up to 6 limbs each
    base = [values(pair, rng, b, l, n) for b, l in small[:4]] + [mask_column(rng, n), mask_column(rng, n)]
    specs, at = [], len(base)
    for k in range(64):
        b, l = small[k % len(small)]
        mask = [None, ("nonzero", 4 + k % 2), ("zero", 4 + (k + 1) % 2)][k % 3]
        specs.append(LimbSpec(k % 4, at, l, b, mask))
        at += l
    base += [[0] * n for _ in range(at - len(base))]
    want, rep, _ = run(kind, fname, base, specs, fname, fill=SENTINEL)
    assert rep["overflow"] > 0 and 0 < rep["active"] < 64 * n


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_all_rows_inactive(kind, fname):
    pair, n = FIELDS[fname], 300
    rng = np.random.default_rng(300)
    base = [values(pair, rng, 16, 3, n), [0] * n] + [[0] * n for _ in range(3)]
    want, rep, report = run(kind, fname, base, [LimbSpec(0, 2, 3, 16, ("nonzero", 1))], fname, fill=SENTINEL)
    assert rep == {"overflow": 0, "first_overflow_spec": 0, "first_overflow_row": 0, "active": 0} and all(v == 0 for c in want[2:] for v in c)
    assert report and report.check() is report and report.first_overflow_value() is None


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_overflow_in_several_specs_reports_the_smallest_spec_and_row(kind, fname):
    pair, n = FIELDS[fname], 600
    rng = np.random.default_rng(600)
    cols = [[int(v) for v in rng.integers(0, 1 << 32, size=n)] for _ in range(3)]
    for c, i in ((1, 599), (1, 258), (2, 0), (2, 300), (1, 257)):
        cols[c][i] = (1 << 32) + i
    cols[0][5] = 1 << 40                                                        # spec 0 reads column 0 masked: row 5 is inactive there
    maskc = [1] * n
    maskc[5] = 0
    base = cols + [maskc] + [[0] * n for _ in range(6)]
    specs = [LimbSpec(0, 4, 2, 16, ("nonzero", 3)), LimbSpec(1, 6, 2, 16), LimbSpec(2, 8, 2, 16)]
    want, rep, report = run(kind, fname, base, specs, fname)
    assert rep == {"overflow": 5, "first_overflow_spec": 1, "first_overflow_row": 257, "active": 3 * n - 1}
    assert want[6][257] == 257 and want[7][257] == 0                            # an overflowing row still gets its low limbs
    assert not report and "overflow=5" in repr(report) and report.first_overflow_value() == (1 << 32) + 257
    with pytest.raises(LookupMissing) as err:
        report.check()
    assert (err.value.spec, err.value.row, err.value.value, err.value.missing) == (1, 257, (1 << 32) + 257, 5)
    assert "spec 1, row 257" in str(err.value) and str((1 << 32) + 257) in str(err.value)


@pytest.mark.gpu
def test_a_lane_takes_a_second_row_past_the_grid_cap():
    """4096 workgroups of 256 lanes is the most stream_grid gives: with 2^20 + 257 rows the first 257 lanes take a second row"""
    pl = backends.planner("hip")
    n, P = (1 << 20) + 257, FIELDS["fp"].bf.p
    rng = np.random.default_rng(20)
    v = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    v[-257:] = np.arange(257, dtype=np.uint64) * np.uint64(0x0001000100010001) + np.uint64(1 << 62)
    v[-3] = np.uint64(P - 1)
    mont = lambda a: np.array((a.astype(object) << 64) % P, dtype=np.uint64)
    cols = [GpuVec.from_numpy(pl, mont(v), FP)] + [GpuVec.from_numpy(pl, np.full(n, SENTINEL, dtype=np.uint64), FP) for _ in range(4)]
    report = limb_decompose(pl, cols, [LimbSpec(0, 1, 4, 16)])
    for j in range(4):
        got, want = cols[1 + j].to_numpy(), mont((v >> np.uint64(16 * j)) & np.uint64(0xFFFF))
        assert np.array_equal(got, want), (j, int(np.nonzero(got != want)[0][0]))
    assert report_dict(report) == {"overflow": 0, "first_overflow_spec": 0, "first_overflow_row": 0, "active": n}


@pytest.mark.gpu
@pytest.mark.parametrize("fname", list(FIELDS))
def test_the_result_is_the_same_on_every_run(fname):
    pl, pair, n = backends.planner("hip"), FIELDS[fname], 4097
    bits, nlimbs = (7, 9) if fname == "fp" else (28, 8)                          # limbs across word boundaries, and fewer bits than the field has
    rng = np.random.default_rng(4097)
    base = [values(pair, rng, bits, nlimbs, n), mask_column(rng, n)] + [[0] * n for _ in range(2 * nlimbs)]
    specs = [LimbSpec(0, 2, nlimbs, bits), LimbSpec(0, 2 + nlimbs, nlimbs, bits, ("zero", 1))]
    want, rep = reference(base, specs)
    assert rep["overflow"] > 100
    runs = []
    for _ in range(3):
        d = upload(pl, fname, base)
        report = limb_decompose(pl, d, specs)
        assert report_dict(report) == rep
        runs.append([c.to_numpy() for c in d.columns] + [report.buf.to_numpy()])
    assert all(np.array_equal(a, words(fname, w)) for a, w in zip(runs[0], want))
    assert all(np.array_equal(a, b) for r in runs[1:] for a, b in zip(runs[0], r))


# ---- refusals and empty cases --------------------------------------------------------------------------------------------------------
class Call:
    """one raw call whose arguments a test can bend: columns 0, 1 sources, 2, 3 masks, 4 .. 9 destinations, all filled with known words"""

    def __init__(self, kind, fname="fp", n=300):
        self.pl, self.pair, self.fname = backends.planner(kind), FIELDS[fname], fname
        rng = np.random.default_rng(n)
        self.base = [values(self.pair, rng, 16, 2, n), values(self.pair, rng, 12, 3, n), mask_column(rng, n), mask_column(rng, n)] + [[SENTINEL % self.pair.bf.p] * n for _ in range(6)]
        self.specs = [[0, 4, 2, 16, 1, 2, 0, 0], [1, 6, 3, 12, 2, 3, 0, 0]]
        self.V = self.pair.bf.nlimbs
        self.cols = [GpuVec.from_numpy(self.pl, words(fname, c) if k < 4 else np.full(n * self.V, SENTINEL, dtype=np.uint64), self.pair.base_field) for k, c in enumerate(self.base)]
        self.report = GpuVec.from_numpy(self.pl, np.full(4, SENTINEL, dtype=np.uint64), FP)
        self.field, self.n, self.nspecs, self.nbase = self.pair.base_field, n, 2, 10
        self.ptrs, self.report_ptr, self.null, self.handle = [c.ptr for c in self.cols], self.report.ptr, (), self.pl.handle

    def __call__(self):
        rec = np.array(self.specs, dtype=np.int32).reshape(-1, 8)
        arr = None if "base" in self.null else (ctypes.c_void_p * len(self.ptrs))(*self.ptrs)
        return self.pl.lib.ms_limb_decompose(self.handle, self.field, self.n, arr, self.nbase, None if "specs" in self.null else rec.ctypes.data, self.nspecs, self.report_ptr)

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self):
        assert all((c.to_numpy() == np.uint64(SENTINEL)).all() for c in self.cols[4:]) and (self.report.to_numpy() == np.uint64(SENTINEL)).all()
        assert all(np.array_equal(c.to_numpy(), words(self.fname, v)) for c, v in zip(self.cols[:4], self.base))

    def record(self):
        rec = LimbReportRecord.from_buffer_copy(self.report.to_numpy().tobytes())
        return {k: int(getattr(rec, k)) for k in LIMB_REPORT_FIELDS}

    def expected(self):
        class S:
            def __init__(s, r):
                s.src, s.dst0, s.nlimbs, s.bits = r[:4]
                s.mask = None if r[4] == 0 else (("nonzero", "zero")[r[4] - 1], r[5])
        return reference(self.base, [S(r) for r in self.specs[:self.nspecs]], self.n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_the_bent_call_is_accepted_unbent(kind, fname):
    call = Call(kind, fname)
    assert call() == 0, call.error()
    want, rep = call.expected()
    assert call.record() == rep and rep["active"] > 0
    for c in range(4, 9):
        assert np.array_equal(call.cols[c].to_numpy(), words(fname, want[c]))
    assert (call.cols[9].to_numpy() == np.uint64(SENTINEL)).all()               # a column that no spec names


@pytest.mark.parametrize("kind", KINDS)
def test_null_arguments_limits_indices_and_mask_kinds_are_refused(kind):
    S = lambda k, w, v: (lambda c: c.specs[k].__setitem__(w, v))
    bends = [(lambda c: setattr(c, "handle", None), "null"), (lambda c: setattr(c, "null", ("base",)), "null"), (lambda c: setattr(c, "null", ("specs",)), "null"),
             (lambda c: setattr(c, "report_ptr", None), "null"), (lambda c: c.ptrs.__setitem__(9, None), "null base column 9"), (lambda c: setattr(c, "field", 7), ""),
             (S(0, 0, 10), "out of range"), (S(1, 0, -1), "out of range"),                              # a source column
             (S(0, 5, 10), "mask"), (S(1, 5, -1), "mask"), (S(0, 4, 3), "mask kind"), (S(1, 4, -1), "mask kind"),
             (S(0, 3, 0), "bits"), (S(0, 3, 33), "bits"), (S(1, 2, 0), "limbs"), (S(1, 2, 257), "limbs"),
             (S(0, 2, 5), "more than the 64 bits"), (S(1, 3, 22), "more than the 64 bits"),             # 5 * 16 and 3 * 22 bits
             (S(0, 1, -1), "out of range"), (S(0, 1, 10), "out of range"), (S(0, 1, 9), "out of range"),               # dst0, and dst0 + nlimbs past the table
             (lambda c: (setattr(c, "nspecs", 65), setattr(c, "specs", c.specs[:1] * 65)), "at most 64"),
             (lambda c: setattr(c, "n", (1 << 32) + 1), "2^32")]
    for k, (bend, text) in enumerate(bends):
        call = Call(kind)
        bend(call)
        assert call() == INVALID and text in call.error(), (k, call.error())
        call.unchanged()
    call = Call(kind)
    call.field = FQ3F
    assert call() == UNSUPPORTED and "Fq3" in call.error(), call.error()
    call.unchanged()
    call = Call(kind, "fp252")                                                  # 256 bits of words: 8 limbs of 32 fit, 9 do not
    call.specs[0][2:4] = [9, 32]
    assert call() == INVALID and "more than the 256 bits" in call.error(), call.error()
    call = Call(kind)                                                           # what is not read is not checked: an unmasked spec's mask column
    call.specs[0][4:6] = [0, 99]
    assert call() == 0, call.error()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_overlaps_are_refused(kind, fname):
    def refused(bend):
        call = Call(kind, fname)
        bend(call)
        assert call() == INVALID and "overlap" in call.error(), call.error()
        call.unchanged()
    S = lambda k, w, v: (lambda c: c.specs[k].__setitem__(w, v))
    col = lambda c: 8 * c.V * c.n
    refused(S(0, 1, 0))                                                         # a destination that is its own source
    refused(S(0, 1, 1))                                                         # ... another spec's source (dst 1, 2)
    refused(S(1, 1, 2))                                                         # ... a mask column of another spec
    refused(S(1, 0, 4))                                                         # a source that another spec writes
    refused(S(1, 5, 5))                                                         # a mask that another spec writes
    refused(S(1, 1, 5))                                                         # destination ranges 4, 5 and 5, 6, 7
    refused(S(1, 1, 3))                                                         # 3 (its own mask), 4, 5
    refused(lambda c: c.ptrs.__setitem__(4, c.ptrs[0]))                         # by address: a destination on a source
    refused(lambda c: c.ptrs.__setitem__(7, c.ptrs[3] + col(c) - 8))            # ... on the last word of a mask column
    refused(lambda c: setattr(c, "report_ptr", c.ptrs[1] + 8))
    refused(lambda c: setattr(c, "report_ptr", c.ptrs[2] + col(c) - 8))
    refused(lambda c: setattr(c, "report_ptr", c.ptrs[8]))                      # a destination is a named column too
    call = Call(kind, fname)                                                    # a column that no spec names may take the report
    call.report_ptr = call.ptrs[9]
    assert call() == 0, call.error()


@pytest.mark.parametrize("kind", KINDS)
def test_no_rows_and_no_specs(kind):
    for bend in (lambda c: setattr(c, "n", 0), lambda c: (setattr(c, "nspecs", 0), setattr(c, "null", ("specs",))), lambda c: (setattr(c, "n", 0), setattr(c, "nspecs", 0))):
        call = Call(kind)
        bend(call)
        assert call() == 0, call.error()
        assert call.record() == {k: 0 for k in LIMB_REPORT_FIELDS}
        assert all((c.to_numpy() == np.uint64(SENTINEL)).all() for c in call.cols[4:])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_checked_mode_names_column_and_row(kind, fname):
    pl, pair = backends.planner(kind), FIELDS[fname]
    p_words = [(pair.bf.p >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(pair.bf.nlimbs)]          # p itself: the smallest non-canonical value
    V = len(p_words)
    try:
        pl.checked(True)
        for col, row in ((0, 17), (1, 299), (2, 0), (3, 150)):                 # the sources and the masks
            call = Call(kind, fname)
            w = words(fname, call.base[col])
            w[V * row:V * (row + 1)] = p_words
            keep = GpuVec.from_numpy(pl, w, pair.base_field)
            call.ptrs[col] = keep.ptr
            assert call() == INVALID, call.error()
            msg = call.error()
            assert "canonical" in msg and "ms_limb_decompose" in msg and "d_base" in msg and f"column {col}, row {row};" in msg, msg
            assert all((c.to_numpy() == np.uint64(SENTINEL)).all() for c in call.cols[4:]) and (call.report.to_numpy() == np.uint64(SENTINEL)).all()
        call = Call(kind, fname)                                                # the destinations hold 0xA5A5.. words, not canonical over Fp252's top word: not scanned
        assert call() == 0, call.error()
        want, rep = call.expected()
        assert call.record() == rep
    finally:
        pl.checked(False)


def test_python_mirror_argument_checks():
    pl = backends.planner("emu")
    d = upload(pl, "fp", [[0x12345678, 7, 1 << 33], [0] * 3, [0] * 3])
    report = limb_decompose(pl, d, [LimbSpec(0, 1, 2, 16)])
    assert list(d.columns[1].to_numpy()) == list(words("fp", [0x5678, 7, 0])) and list(d.columns[2].to_numpy()) == list(words("fp", [0x1234, 0, 0]))
    assert (report.overflow, report.first_overflow_spec, report.first_overflow_row, report.active) == (1, 0, 2, 3)
    with pytest.raises(MsError) as err:
        limb_decompose(pl, d, [LimbSpec(0, 0, 2, 16)])
    assert err.value.code == INVALID and "overlap" in str(err.value)
    with pytest.raises(MsError) as err:
        limb_decompose(pl, d, [LimbSpec(0, 2, 2, 16)])
    assert err.value.code == INVALID and "out of range" in str(err.value)
    for bad in (lambda: LimbSpec(0, 1, 2, 33), lambda: LimbSpec(0, 1, 0, 8), lambda: LimbSpec(0, 1, 257, 1), lambda: LimbSpec(0, 1, 2, 16, ("odd", 1)),
                lambda: limb_decompose(pl, d, [LimbSpec(0, 1, 3, 32)]), lambda: limb_decompose(pl, d, [LimbSpec(0, 1, 1, 8)] * 65),
                lambda: limb_decompose(pl, [d.columns[0], GpuVec(pl, 2, FP)], [])):
        with pytest.raises(ValueError):
            bad()
    assert (extension.RANGE_MAX_SPECS, extension.RANGE_MAX_LIMBS, extension.RANGE_MAX_LIMB_BITS) == (64, 256, 32)
    assert limb_decompose(pl, d, []).active == 0
