"""ms_bitwise_columns (include/ministark_hip_bitwise.h) against the loop on Python integers (tests/bitwise_ref.py): both fields, the three
ops under the three masks in mixed specs, every width class (one bit, a word's edge over Fp252, WMAX), row counts around a workgroup,
operands at W - 1, W, p - 1 and 252-bit operands whose low word alone is in range, 64 specs in one call, a == b, unread columns left as
they are, inactive rows zero, the report field for field -- and the refusals, after which the sentinel-filled outputs are unchanged."""
import ctypes
import functools

import numpy as np
import pytest

from tests import backends
from tests.bitwise_ref import LIMB_REPORT_FIELDS, bitwise_columns as reference
from tests.ext_ref import PAIRS
from ministark_amd import BitwiseSpec, GpuVec, LimbReport, LookupMissing, Matrix, bitwise_columns
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F
from ministark_amd._lib import LimbReportRecord, MsError

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = {"fp": PAIRS["fp_fp"], "fp252": PAIRS["fp252_fp252"]}
WIDTHS = {"fp": [1, 8, 32, 63], "fp252": [1, 64, 65, 128, 251]}
WMAX = {"fp": 63, "fp252": 251}
OPS = ["and", "or", "xor"]
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


def below(rng, width, n):
    """n integers below 2^width, every bit drawn"""
    out = [0] * n
    for k in range(0, width, 32):
        out = [v | (int(r) & ((1 << min(32, width - k)) - 1)) << k for v, r in zip(out, rng.integers(0, 1 << 32, size=n))]
    return out


def operands(pair, rng, width, n, shift):
    """operands below W = 2^width, and at the edges: W - 1, W, p - 1, and over Fp252 values whose low word alone is in range"""
    W, vals = 1 << width, below(rng, width, n)
    edges = [W - 1, W, pair.bf.p - 1, 0, W + 1]
    if pair.bf.nlimbs == 4:
        edges += [(1 << 64) + 1, (1 << 128) + (W - 1) % (1 << 64), (1 << 192) + 2, (1 << 251) + 1]
    for k, e in enumerate(edges[:n]):
        vals[(7 * k + shift) % n] = e % pair.bf.p
    return vals


def report_dict(report):
    return {k: getattr(report, k) for k in LIMB_REPORT_FIELDS}


def run(kind, fname, base, specs, what):
    pl = backends.planner(kind)
    want, rep = reference(base, specs)
    d = upload(pl, fname, base)
    report = bitwise_columns(pl, d, specs)
    assert isinstance(report, LimbReport)
    for k, (c, v) in enumerate(zip(d.columns, want)):
        got, exp = c.to_numpy(), words(fname, v)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (what, f"column {k}: {bad.size} words differ, the first is word {int(bad[0])}")
    assert report_dict(report) == rep, what
    return want, rep, report


def mixed(fname, n, seed):
    """columns [a_w, b_w for every width | mask | spare | one dst per spec]; per width the three ops, the mask kinds turning"""
    pair, widths = FIELDS[fname], WIDTHS[fname]
    rng = np.random.default_rng([seed, n])
    base = []
    for w in widths:
        base += [operands(pair, rng, w, n, 3), operands(pair, rng, w, n, 5)]
    mcol, spare = len(base), len(base) + 1
    base += [mask_column(rng, n), [SENTINEL % pair.bf.p] * n]
    masks = [None, ("nonzero", mcol), ("zero", mcol)]
    specs = []
    for k, w in enumerate(widths):
        for o, op in enumerate(OPS):
            specs.append(BitwiseSpec(op, 2 * k, 2 * k + 1, len(base), w, masks[(k + o) % 3]))
            base.append([(SENTINEL + len(base)) % pair.bf.p] * n)
    return base, specs, spare


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2500])
def test_mixed_specs_at_every_width(kind, fname, n):
    base, specs, spare = mixed(fname, n, 1)
    want, rep, report = run(kind, fname, base, specs, (fname, n))
    assert want[spare] == base[spare]                                           # a column no spec names stays as it is
    if n >= 255:
        assert 0 < rep["overflow"] < rep["active"] < n * len(specs)
        sp = next(sp for sp in specs if sp.mask and sp.mask[0] == "nonzero")    # an inactive row is zero, whatever the column held
        assert all(want[sp.dst][i] == 0 for i in range(n) if base[sp.mask[1]][i] == 0) and any(v == 0 for v in base[sp.mask[1]])
        with pytest.raises(LookupMissing) as err:
            report.check()
        k, row = rep["first_overflow_spec"], rep["first_overflow_row"]
        assert (err.value.spec, err.value.row, err.value.values) == (k, row, [base[specs[k].a][row], base[specs[k].b][row]])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_sixty_four_specs_and_an_operand_with_itself(kind, fname):
    pair, n, wmax = FIELDS[fname], 257, WMAX[fname]
    rng = np.random.default_rng(64)
    base = [operands(pair, rng, wmax, n, c) for c in range(3)] + [mask_column(rng, n)]
    specs = []
    for k in range(64):
        a, b = k % 3, (k % 3) if k % 4 == 0 else (k + 1) % 3                     # a == b: x and x = x or x = x, x xor x = 0
        specs.append(BitwiseSpec(k % 3, a, b, 4 + k, 1 + (k * 37) % wmax, [None, ("nonzero", 3), ("zero", 3)][k % 3]))
    base += [[1] * n for _ in range(64)]
    want, rep, _ = run(kind, fname, base, specs, fname)
    xor_self = [k for k, sp in enumerate(specs) if sp.a == sp.b and sp.op == 2]
    assert xor_self and all(set(want[4 + k]) == {0} for k in xor_self) and rep["overflow"] > 0


# ---- refusals and empty cases --------------------------------------------------------------------------------------------------------
class Call:
    """one raw call whose arguments a test can bend: columns 0, 1 operands, 2 a mask, 3, 4 destinations, 5 spare; the destinations, the
    spare column and d_report hold a sentinel"""

    def __init__(self, kind, fname="fp", n=300):
        self.pl, self.pair, self.fname = backends.planner(kind), FIELDS[fname], fname
        rng = np.random.default_rng(n)
        sent = SENTINEL % self.pair.bf.p
        self.base = [operands(self.pair, rng, 20, n, 3), operands(self.pair, rng, 20, n, 5), mask_column(rng, n), [sent] * n, [sent] * n, [sent] * n]
        self.specs = [[0, 0, 1, 3, 20, 1, 2, 0], [2, 1, 0, 4, 20, 0, 0, 0]]      # op, a, b, dst, width, mask, mask_col, pad
        self.V = self.pair.bf.nlimbs
        self.cols = [GpuVec.from_numpy(self.pl, words(fname, c), self.pair.base_field) for c in self.base]
        self.report = GpuVec.from_numpy(self.pl, np.full(4, SENTINEL, dtype=np.uint64), FP)
        self.field, self.n, self.nspecs, self.nbase = self.pair.base_field, n, 2, 6
        self.ptrs, self.report_ptr, self.null, self.handle = [c.ptr for c in self.cols], self.report.ptr, (), self.pl.handle

    def __call__(self):
        rec = np.array(self.specs, dtype=np.int32).reshape(-1, 8)
        arr = None if "base" in self.null else (ctypes.c_void_p * len(self.ptrs))(*self.ptrs)
        return self.pl.lib.ms_bitwise_columns(self.handle, self.field, self.n, arr, self.nbase, None if "specs" in self.null else rec.ctypes.data, self.nspecs, self.report_ptr)

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self, report=True):
        for c, v in zip(self.cols, self.base):
            assert np.array_equal(c.to_numpy(), words(self.fname, v))
        assert not report or (self.report.to_numpy() == np.uint64(SENTINEL)).all()

    def record(self):
        rec = LimbReportRecord.from_buffer_copy(self.report.to_numpy().tobytes())
        return {k: int(getattr(rec, k)) for k in LIMB_REPORT_FIELDS}

    def expected(self):
        mk = lambda r: None if r[5] == 0 else (("nonzero", "zero")[r[5] - 1], r[6])
        return reference(self.base, [BitwiseSpec(r[0], r[1], r[2], r[3], r[4], mk(r)) for r in self.specs[:self.nspecs]])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_the_bent_call_is_accepted_unbent(kind, fname):
    call = Call(kind, fname)
    assert call() == 0, call.error()
    want, rep = call.expected()
    for c, v in zip(call.cols, want):
        assert np.array_equal(c.to_numpy(), words(fname, v))
    assert call.record() == rep and rep["overflow"] > 0 and want[5] == call.base[5]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_limits_indices_and_overlaps_are_refused(kind, fname):
    S = lambda k, w, v: (lambda c: c.specs[k].__setitem__(w, v))
    col = lambda c: 8 * c.V * c.n
    bends = [(lambda c: setattr(c, "handle", None), "null"), (lambda c: setattr(c, "null", ("base",)), "null"), (lambda c: setattr(c, "null", ("specs",)), "null"),
             (lambda c: setattr(c, "report_ptr", None), "null"), (lambda c: c.ptrs.__setitem__(5, None), "null base column 5"),
             (S(0, 4, 0), "bits"), (S(1, 4, WMAX[fname] + 1), "bits"), (S(0, 0, 3), "unknown op"), (S(1, 0, -1), "unknown op"),
             (S(0, 1, 6), "out of range"), (S(1, 2, -1), "out of range"), (S(0, 3, 6), "out of range"), (S(0, 6, 6), "mask"), (S(0, 5, 3), "mask kind"),
             (S(0, 3, 0), "overlap"), (S(0, 3, 1), "overlap"), (S(1, 3, 2), "overlap"),            # dst = an operand, = the mask of ANOTHER spec
             (S(1, 3, 3), "overlap"),                                                             # two specs with one dst
             (lambda c: c.ptrs.__setitem__(4, c.ptrs[0] + col(c) - 8), "overlap"),                # a dst whose memory overlaps an operand's last word
             (lambda c: setattr(c, "report_ptr", c.ptrs[1] + 8), "overlap"), (lambda c: setattr(c, "report_ptr", c.ptrs[2] + col(c) - 8), "overlap"),
             (lambda c: setattr(c, "report_ptr", c.ptrs[3]), "overlap"),
             (lambda c: (setattr(c, "nspecs", 65), setattr(c, "specs", c.specs[:1] * 65)), "65 specs"), (lambda c: setattr(c, "n", (1 << 32) + 1), "rows")]
    for k, (bend, text) in enumerate(bends):
        call = Call(kind, fname)
        bend(call)
        assert call() == INVALID and text in call.error(), (k, call.error())
        call.unchanged()
    call = Call(kind, fname)
    call.field = FQ3F
    assert call() == UNSUPPORTED, call.error()
    call.unchanged()
    call = Call(kind, fname)                                                    # the widest operand is accepted
    call.specs[1][4] = WMAX[fname]
    assert call() == 0, call.error()
    assert call.record() == call.expected()[1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_no_rows_and_no_specs(kind, fname):
    for bend in (lambda c: setattr(c, "n", 0), lambda c: (setattr(c, "nspecs", 0), setattr(c, "null", ("specs",))), lambda c: (setattr(c, "n", 0), setattr(c, "nspecs", 0))):
        call = Call(kind, fname)
        bend(call)
        assert call() == 0, call.error()
        call.unchanged(report=False)
        assert call.record() == {k: 0 for k in LIMB_REPORT_FIELDS}


@pytest.mark.parametrize("kind", KINDS)
def test_checked_mode_scans_what_is_read_and_not_the_destinations(kind):
    pl = backends.planner(kind)
    try:
        pl.checked(True)
        call = Call(kind)
        bad = GpuVec.from_numpy(pl, np.full(call.n, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), FP)
        call.ptrs[1] = bad.ptr
        assert call() == INVALID and "canonical" in call.error() and "column 1, row 0;" in call.error(), call.error()
        call.unchanged()
        call = Call(kind)
        call.ptrs[3] = bad.ptr                                                  # a destination may hold anything
        assert call() == 0, call.error()
        want, rep = call.expected()
        assert np.array_equal(bad.to_numpy(), words("fp", want[3])) and call.record() == rep
    finally:
        pl.checked(False)


def test_python_mirror_argument_checks():
    pl = backends.planner("emu")
    d = upload(pl, "fp", [[12, 5, 255, 256], [10, 3, 15, 1], [7, 7, 7, 7]])
    report = bitwise_columns(pl, d, [BitwiseSpec("xor", 0, 1, 2, 8)])
    assert list(d.columns[2].to_numpy()) == list(words("fp", [6, 6, 240, 1]))
    assert (report.overflow, report.first_overflow_spec, report.first_overflow_row, report.active, report.first_overflow_value()) == (1, 0, 3, 4, (256, 1))
    assert bitwise_columns(pl, d, []).check().active == 0
    with pytest.raises(MsError) as err:
        bitwise_columns(pl, d, [BitwiseSpec("and", 0, 1, 1, 8)])
    assert err.value.code == INVALID and "overlap" in str(err.value)
    for bad in (lambda: BitwiseSpec("nand", 0, 1, 2, 8), lambda: BitwiseSpec(3, 0, 1, 2, 8), lambda: BitwiseSpec("and", 0, 1, 2, 0), lambda: BitwiseSpec("and", 0, 1, 2, 252),
                lambda: bitwise_columns(pl, d, [BitwiseSpec("and", 0, 1, 2, 64)]), lambda: bitwise_columns(pl, d, [BitwiseSpec("and", 0, 1, 2, 8)] * 65),
                lambda: BitwiseSpec("or", 0, 1, 2, 8, ("odd", 1))):
        with pytest.raises(ValueError):
            bad()
