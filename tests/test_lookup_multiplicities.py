"""ms_lookup_multiplicities (include/ministark_hip_lookup.h) against the loop on Python integers (tests/lookup_ref.py), m and report word
for word: lengths around the rows of a workgroup and of the grid-stride, widths 1..4, both fields, 1..3 sets, the three masks on table and
lookups, tables so small that the probe walk wraps, the sequential-key table, keys that differ in one word only (every component, every
limb), the all-equal table, every lookup into one row, missing tuples in several sets, the output as a column of the base table -- and the
refusals, after which the sentinel-filled d_m and d_report are unchanged.  What only the device can show -- that the atomics lose nothing
and that the result does not depend on the order of the inserts -- is the `hip` half of every case and the determinism test."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import backends
from tests.ext_ref import PAIRS
from tests.lookup_ref import reference
from ministark_amd import GpuVec, LookupMissing, LookupTuple, Matrix, extension, lookup_multiplicities
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, STARK252_FP as F252F
from ministark_amd._lib import LookupReportRecord, MsError

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = {"fp": PAIRS["fp_fp"], "fp252": PAIRS["fp252_fp252"]}
LENGTHS = [1, 2, 3, 255, 256, 257, 1025, 4097]
INVALID, UNSUPPORTED = -1, -2
SENTINEL = 0xA5A5A5A5A5A5A5A5
REPORT_FIELDS = ("missing", "first_missing_set", "first_missing_row", "duplicate_table_rows")
MASKS = [None, "nonzero", "zero"]


def rand_values(pair, rng, count):
    if pair.bf.nlimbs == 1:
        return [int(v) for v in rng.integers(0, pair.bf.p, size=count, dtype=np.uint64)]
    return [int.from_bytes(rng.bytes(32), "little") % pair.bf.p for _ in range(count)]


def layout(width, nsets, table_mask=None, lookup_masks=None):
    """base columns: the table's `width`, then every set's, then two mask columns, then the column for m.
    -> (table, lookups, nbase, index of the m column)"""
    mask_a, mask_b, out = width * (1 + nsets), width * (1 + nsets) + 1, width * (1 + nsets) + 2
    mk = lambda kind, col: None if kind is None else (kind, col)
    table = LookupTuple(range(width), mk(table_mask, mask_a))
    lookups = [LookupTuple(range(width * (1 + s), width * (2 + s)), mk((lookup_masks or [None] * nsets)[s], mask_b if s % 2 == 0 else mask_a)) for s in range(nsets)]
    return table, lookups, out + 1, out


@functools.lru_cache(maxsize=None)
def case(fname, n, width, nsets, npool, table_mask=None, lookup_masks=None, seed=0):
    """(base columns as integers, table, lookups, m column index, expected counts, expected report), computed once and shared by the backends.
    The table's rows are drawn from a pool of `npool` tuples (npool < n: equal rows); a lookup row is drawn from the pool and from as many
    foreign tuples again, so about half the pool's tuples that the table happens not to hold, and every foreign one, are missing."""
    pair = FIELDS[fname]
    rng = np.random.default_rng([n, width, nsets, npool, seed])
    table, lookups, nbase, out = layout(width, nsets, table_mask, lookup_masks)
    vals = rand_values(pair, rng, 2 * npool * width)
    pool = [tuple(vals[k * width:(k + 1) * width]) for k in range(2 * npool)]
    base = [[0] * n for _ in range(nbase)]
    for j, k in enumerate(rng.integers(0, npool, size=n)):
        for c in range(width):
            base[c][j] = pool[k][c]
    for s in range(nsets):
        for i, k in enumerate(rng.integers(0, npool + max(1, npool // 8), size=n)):
            for c in range(width):
                base[width * (1 + s) + c][i] = pool[k][c]
    for col in (out - 2, out - 1):
        base[col] = [int(v) if k else 0 for v, k in zip(rng.integers(1, 1 << 62, size=n), rng.integers(0, 3, size=n))]
    base[out] = [SENTINEL % pair.bf.p] * n
    cnt, rep = reference(base, table, lookups)
    return base, table, lookups, out, cnt, rep


def upload(pl, pair, base):
    return Matrix([GpuVec.from_numpy(pl, pair.base_words(c), pair.base_field) for c in base])


def check(pair, m, report, cnt, rep, what):
    got = m.to_numpy()
    want = pair.base_words(cnt)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, f"{bad.size} words of m differ, the first in row {int(bad[0]) // pair.bf.nlimbs}")
    assert {k: getattr(report, k) for k in REPORT_FIELDS} == rep, what


def run_case(kind, fname, *args, in_place=True, **kw):
    pl, pair = backends.planner(kind), FIELDS[fname]
    base, table, lookups, out, cnt, rep = case(fname, *args, **kw)
    d_base = upload(pl, pair, base)
    m, report = lookup_multiplicities(pl, d_base, table, lookups, out=d_base.columns[out] if in_place else None)
    check(pair, m, report, cnt, rep, (fname, args, kw))
    for c, v in list(zip(d_base.columns, base))[:out]:                        # the inputs are only read
        assert np.array_equal(c.to_numpy(), pair.base_words(v))
    return rep


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_and_widths(kind, fname, n):
    """every length at every width; the number of sets and the masks go round with the width.  m is the base table's own last column."""
    for width in (1, 2, 3, 4):
        nsets = 1 + width % 3
        run_case(kind, fname, n, width, nsets, max(1, n // 2), MASKS[width % 3], tuple(MASKS[(width + s) % 3] for s in range(nsets)))


@pytest.mark.parametrize("kind", KINDS)
def test_two_hundred_tables_of_at_most_eight_rows(kind):
    """capacities 2 .. 16: the probe walk wraps round the end of the slot array"""
    pl = backends.planner(kind)
    rng = np.random.default_rng(8)
    seen_missing = seen_dups = 0
    for k in range(200):
        fname = ("fp", "fp252")[k % 2]
        pair = FIELDS[fname]
        n, width, nsets = int(rng.integers(1, 9)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
        table, lookups, nbase, out = layout(width, nsets, MASKS[k % 3] if k % 5 == 0 else None)
        base = [[int(v) for v in rng.integers(0, 3, size=n)] for _ in range(nbase)]          # values 0, 1, 2: every kind of coincidence
        cnt, rep = reference(base, table, lookups)
        m, report = lookup_multiplicities(pl, upload(pl, pair, base), table, lookups)
        check(pair, m, report, cnt, rep, (k, fname, n, width, nsets, base))
        seen_missing += rep["missing"] > 0
        seen_dups += rep["duplicate_table_rows"] > 0
    assert seen_missing > 20 and seen_dups > 20


@functools.lru_cache(maxsize=None)
def sequential_case(n):
    rng = np.random.default_rng(n)
    base = [list(range(n)), [int(v) for v in rng.integers(0, n, size=n)], [0] * n]
    table, lookups = LookupTuple([0]), [LookupTuple([1])]
    return base, table, lookups, reference(base, table, lookups)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_the_sequential_key_table(kind, fname):
    pl, pair = backends.planner(kind), FIELDS[fname]
    base, table, lookups, (cnt, rep) = sequential_case(4096)
    assert rep["missing"] == 0 and rep["duplicate_table_rows"] == 0 and sum(cnt) == 4096
    m, report = lookup_multiplicities(pl, upload(pl, pair, base), table, lookups)
    check(pair, m, report, cnt, rep, fname)


def limbs_to_words(residues, nlimbs):
    return np.array([(r >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for r in residues for k in range(nlimbs)], dtype=np.uint64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_keys_that_differ_in_one_word_only(kind, fname, width):
    """Residues are uploaded as they are (all below p, so canonical): row 0 of the table is a tuple K, row 1 + v the same tuple with one bit
    of ONE word flipped -- every component, every limb.  A compare that skips that word takes the row for a duplicate of row 0; variant v is
    looked up v + 2 times and K once, so every row's m tells the rows apart."""
    pl, pair = backends.planner(kind), FIELDS[fname]
    L = pair.bf.nlimbs
    rng = np.random.default_rng(width)
    K = [int.from_bytes(rng.bytes(8 * L - 2), "little") for _ in range(width)]                # below 2^(64 L - 16) < p
    rows = [tuple(K)] + [tuple(x ^ (1 << (64 * l + 7)) if c == cc else x for cc, x in enumerate(K)) for c in range(width) for l in range(L)]
    assert len(set(rows)) == 1 + width * L and all(x < pair.bf.p for r in rows for x in r)
    looked = [r for v, r in enumerate(rows) for _ in range(v + 1 if v == 0 else v + 2)]
    n = len(looked)
    filler = [tuple(int.from_bytes(rng.bytes(8 * L - 2), "little") for _ in range(width)) for _ in range(n - len(rows))]
    order = rng.permutation(n)
    base = [[(rows + filler)[j][c] for j in range(n)] for c in range(width)] + [[looked[k][c] for k in order] for c in range(width)]
    table, lookups = LookupTuple(range(width)), [LookupTuple(range(width, 2 * width))]
    cnt, rep = reference(base, table, lookups)
    assert cnt[:len(rows)] == [1] + [v + 2 for v in range(1, len(rows))] and rep["missing"] == 0 and rep["duplicate_table_rows"] == 0
    d_base = Matrix([GpuVec.from_numpy(pl, limbs_to_words(c, L), pair.base_field) for c in base])
    m, report = lookup_multiplicities(pl, d_base, table, lookups)
    check(pair, m, report, cnt, rep, (fname, width))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_a_table_whose_rows_are_all_equal(kind, fname):
    """every insert meets the same slot; row 0 takes all the credit and the other 1023 rows are duplicates"""
    pl, pair = backends.planner(kind), FIELDS[fname]
    n = 1024
    base = [[7] * n, [9] * n, [7] * (n - 3) + [8] * 3, [9] * n]
    table, lookups = LookupTuple([0, 1]), [LookupTuple([2, 3])]
    cnt, rep = reference(base, table, lookups)
    assert cnt == [n - 3] + [0] * (n - 1) and rep == {"missing": 3, "first_missing_set": 0, "first_missing_row": n - 3, "duplicate_table_rows": n - 1}
    m, report = lookup_multiplicities(pl, upload(pl, pair, base), table, lookups)
    check(pair, m, report, cnt, rep, fname)


@pytest.mark.parametrize("kind", KINDS)
def test_every_lookup_into_one_row(kind):
    """one 32-bit counter takes 2^17 adds"""
    pl, pair = backends.planner(kind), FIELDS["fp"]
    n, hot = 1 << 17, 77_777
    rng = np.random.default_rng(17)
    t = np.unique(rng.integers(0, pair.bf.p, size=2 * n, dtype=np.uint64))[:n]
    rng.shuffle(t)
    table_words = (t.astype(object) * ((1 << 64) % pair.bf.p) % pair.bf.p).astype(np.uint64)  # to Montgomery form
    d_base = Matrix([GpuVec.from_numpy(pl, table_words, FP), GpuVec.from_numpy(pl, np.full(n, table_words[hot], dtype=np.uint64), FP)])
    m, report = lookup_multiplicities(pl, d_base, LookupTuple([0]), [LookupTuple([1])])
    want = np.zeros(n, dtype=np.uint64)
    want[hot] = pair.base_words([n])[0]
    assert np.array_equal(m.to_numpy(), want)
    assert {k: getattr(report, k) for k in REPORT_FIELDS} == {"missing": 0, "first_missing_set": 0, "first_missing_row": 0, "duplicate_table_rows": 0}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("nsets", [1, 2, 3])
def test_masks_and_sets(kind, fname, nsets):
    for table_mask in MASKS:
        for lookup_mask in MASKS:
            run_case(kind, fname, 300, 2, nsets, 40, table_mask, (lookup_mask,) + (None, "zero")[:nsets - 1], in_place=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_a_masked_out_table_row_is_not_in_the_table(kind, fname):
    pl, pair = backends.planner(kind), FIELDS[fname]
    #        table      looked up   table mask   lookup mask
    base = [[5, 6, 7, 6], [6, 7, 5, 5], [1, 0, 1, 1], [0, 0, 0, 4]]
    table, lookups = LookupTuple([0], ("nonzero", 2)), [LookupTuple([1], ("zero", 3))]
    cnt, rep = reference(base, table, lookups)
    # row 1 of the table (6) is masked out, but row 3 holds 6 too and is active; the looked-up 5 of row 3 is masked out
    assert cnt == [1, 0, 1, 1] and rep["missing"] == 0
    m, report = lookup_multiplicities(pl, upload(pl, pair, base), table, lookups)
    check(pair, m, report, cnt, rep, fname)
    base[2][3] = 0                                                              # now no active table row holds 6
    cnt, rep = reference(base, table, lookups)
    assert cnt == [1, 0, 1, 0] and rep == {"missing": 1, "first_missing_set": 0, "first_missing_row": 0, "duplicate_table_rows": 0}
    m, report = lookup_multiplicities(pl, upload(pl, pair, base), table, lookups)
    check(pair, m, report, cnt, rep, fname)
    with pytest.raises(LookupMissing) as err:
        report.check()
    assert (err.value.set, err.value.row, err.value.values, err.value.missing) == (0, 0, [6], 1) and "set 0, row 0" in str(err.value) and "(6)" in str(err.value)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_missing_tuples_in_several_sets(kind, fname):
    pl, pair = backends.planner(kind), FIELDS[fname]
    n = 600
    rng = np.random.default_rng(600)
    t = [rand_values(pair, rng, n) for _ in range(2)]
    sets = []
    for s in range(3):
        idx = rng.integers(0, n, size=n)
        sets.append([[t[0][j] for j in idx], [t[1][j] for j in idx]])
    # the first component of a pair alone is in the table, the second alone too: the pair is not
    for s, i in ((1, 599), (1, 258), (2, 0), (2, 300), (1, 257)):
        sets[s][1][i] = t[1][(t[0].index(sets[s][0][i]) + 1) % n]
    base = t + [c for st in sets for c in st]
    table, lookups = LookupTuple([0, 1]), [LookupTuple([2, 3]), LookupTuple([4, 5]), LookupTuple([6, 7])]
    cnt, rep = reference(base, table, lookups)
    assert rep == {"missing": 5, "first_missing_set": 1, "first_missing_row": 257, "duplicate_table_rows": 0} and sum(cnt) == 3 * n - 5
    m, report = lookup_multiplicities(pl, upload(pl, pair, base), table, lookups)
    check(pair, m, report, cnt, rep, fname)
    assert not report and "missing=5" in repr(report)
    with pytest.raises(LookupMissing) as err:
        report.check()
    assert (err.value.set, err.value.row, err.value.values) == (1, 257, [base[4][257], base[5][257]])


@pytest.mark.gpu
@pytest.mark.parametrize("fname", list(FIELDS))
def test_the_result_is_the_same_on_every_run(fname):
    """4097 rows drawn from 64 tuples, three sets: inserts race for the same slots and lookups for the same counters.  Twice in one process:
    the same m, the same report, and both the reference's -- and the same again from the form without the wave-level add."""
    pl, pair = backends.planner("hip"), FIELDS[fname]
    base, table, lookups, out, cnt, rep = case(fname, 4097, 2, 3, 64, None, (None, "nonzero", "zero"))
    assert rep["duplicate_table_rows"] >= 4097 - 64 and rep["missing"] > 100
    d_base = upload(pl, pair, base)
    runs = []
    for plain in (False, False, True):                                          # the third run: one atomicAdd per lookup row, not one per wave and row
        if plain:
            os.environ["MS_LOOKUP_PLAIN_ADDS"] = "1"
        try:
            m, report = lookup_multiplicities(pl, d_base, table, lookups)
        finally:
            os.environ.pop("MS_LOOKUP_PLAIN_ADDS", None)
        check(pair, m, report, cnt, rep, (fname, plain))
        runs.append((m.to_numpy(), report.buf.to_numpy()))
    assert all(np.array_equal(runs[0][0], r[0]) and np.array_equal(runs[0][1], r[1]) for r in runs[1:])


# ---- refusals and empty cases --------------------------------------------------------------------------------------------------------
class Call:
    """one raw call whose arguments a test can bend; d_m and d_report are filled with a sentinel"""

    def __init__(self, kind, fname="fp", n=300):
        self.pl, self.pair = backends.planner(kind), FIELDS[fname]
        base, table, lookups, out, _, _ = case(fname, n, 2, 2, 40, "nonzero", ("zero", None))
        self.d_base = upload(self.pl, self.pair, base[:out])
        self.field, self.n, self.width, self.nsets = self.pair.base_field, n, 2, 2
        self.base_ptrs = [c.ptr for c in self.d_base.columns]
        self.table, self.lookups = table._record(), [t._record() for t in lookups]
        self.V = self.pair.bf.nlimbs
        self.m = GpuVec.from_numpy(self.pl, np.full(n * self.V, SENTINEL, dtype=np.uint64), self.field)
        self.report = GpuVec.from_numpy(self.pl, np.full(4, SENTINEL, dtype=np.uint64), FP)
        self.m_ptr, self.report_ptr, self.null, self.handle = self.m.ptr, self.report.ptr, (), self.pl.handle

    def __call__(self):
        trec = np.array(self.table, dtype=np.int32)
        lrec = np.array(self.lookups, dtype=np.int32).reshape(-1, 8)
        VP = ctypes.c_void_p
        return self.pl.lib.ms_lookup_multiplicities(self.handle, self.field, self.n,
                                                    None if "base" in self.null else (VP * max(1, len(self.base_ptrs)))(*self.base_ptrs), len(self.base_ptrs), self.width,
                                                    None if "table" in self.null else trec.ctypes.data, None if "lookups" in self.null else lrec.ctypes.data,
                                                    self.nsets, self.m_ptr, self.report_ptr)

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self):
        assert (self.m.to_numpy() == np.uint64(SENTINEL)).all() and (self.report.to_numpy() == np.uint64(SENTINEL)).all()


@pytest.mark.parametrize("kind", KINDS)
def test_the_bent_call_is_accepted_unbent(kind):
    call = Call(kind)
    assert call() == 0, call.error()
    assert not (call.m.to_numpy() == np.uint64(SENTINEL)).any() and not (call.report.to_numpy() == np.uint64(SENTINEL)).any()


@pytest.mark.parametrize("kind", KINDS)
def test_null_arguments_widths_indices_and_mask_kinds_are_refused(kind):
    nbase = 8
    bends = [lambda c: setattr(c, "handle", None), lambda c: setattr(c, "null", ("base",)), lambda c: setattr(c, "null", ("table",)),
             lambda c: setattr(c, "null", ("lookups",)), lambda c: setattr(c, "m_ptr", None), lambda c: setattr(c, "report_ptr", None),
             lambda c: c.base_ptrs.__setitem__(5, None), lambda c: setattr(c, "field", 7),
             lambda c: setattr(c, "width", 0), lambda c: setattr(c, "width", 5),
             lambda c: c.table.__setitem__(1, nbase), lambda c: c.table.__setitem__(0, -1), lambda c: c.lookups[1].__setitem__(0, nbase),     # a column
             lambda c: c.table.__setitem__(5, nbase), lambda c: c.lookups[0].__setitem__(5, -1),                                            # a mask column
             lambda c: c.table.__setitem__(4, 3), lambda c: c.lookups[0].__setitem__(4, -1)]                                                # a mask kind
    for k, bend in enumerate(bends):
        call = Call(kind)
        assert len(call.base_ptrs) == nbase
        bend(call)
        assert call() == INVALID, (k, call.error())
        call.unchanged()
    call = Call(kind)                                                           # what is not read is not checked: the components past the width, an unmasked tuple's mask column
    call.table[2], call.table[3], call.lookups[1][5] = 99, -7, 99
    assert call() == 0, call.error()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_overlapping_outputs_are_refused(kind, fname):
    def refused(bend):
        call = Call(kind, fname)
        bend(call)
        assert call() == INVALID and "overlap" in call.error(), call.error()
        call.unchanged()
    col = lambda c: 8 * c.V * c.n
    refused(lambda c: setattr(c, "m_ptr", c.base_ptrs[0]))                     # a table column
    refused(lambda c: setattr(c, "m_ptr", c.base_ptrs[5]))                     # a looked-up column
    refused(lambda c: setattr(c, "m_ptr", c.base_ptrs[6]))                     # a mask column
    refused(lambda c: setattr(c, "m_ptr", c.base_ptrs[3] + col(c) - 8))        # the last word of one
    refused(lambda c: setattr(c, "report_ptr", c.base_ptrs[1] + 8))
    refused(lambda c: setattr(c, "report_ptr", c.m_ptr))                       # each other
    refused(lambda c: setattr(c, "report_ptr", c.m_ptr + col(c) - 8))
    call = Call(kind, fname)                                                    # mask column 7 is named by no tuple of this call: it may take m
    assert call.table[5] == 6 and call.lookups[0][5] == 7 and call.lookups[1][4] == 0
    call.lookups[0][4] = 0
    call.m_ptr = call.base_ptrs[7]
    assert call() == 0, call.error()


@pytest.mark.parametrize("kind", KINDS)
def test_what_is_too_large_and_fq3_are_unsupported(kind):
    for bend in (lambda c: (setattr(c, "nsets", 9), setattr(c, "lookups", c.lookups[:1] * 9)), lambda c: setattr(c, "field", FQ3F),
                 lambda c: setattr(c, "n", (1 << 30) + 1), lambda c: (setattr(c, "n", 1 << 30), setattr(c, "nsets", 4), setattr(c, "lookups", c.lookups * 2))):
        call = Call(kind)
        bend(call)
        assert call() == UNSUPPORTED, call.error()
        call.unchanged()
    call = Call(kind)                                                           # eight sets are accepted
    call.nsets, call.lookups = 8, call.lookups * 4
    assert call() == 0, call.error()


@pytest.mark.parametrize("kind", KINDS)
def test_no_rows_and_no_sets(kind):
    call = Call(kind)
    call.n = 0
    assert call() == 0, call.error()
    assert (call.m.to_numpy() == np.uint64(SENTINEL)).all() and not call.report.to_numpy().any()      # a zero report and nothing else
    call = Call(kind)
    call.nsets, call.null = 0, ("lookups",)
    assert call() == 0, call.error()
    rec = LookupReportRecord.from_buffer_copy(call.report.to_numpy().tobytes())
    base, table, _, _, _, _ = case("fp", 300, 2, 2, 40, "nonzero", ("zero", None))
    assert not call.m.to_numpy().any() and rec.missing == 0 and rec.duplicate_table_rows == reference(base, table, [])[1]["duplicate_table_rows"] > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_checked_mode_names_argument_column_and_row(kind, fname):
    pl, pair = backends.planner(kind), FIELDS[fname]
    n = 300
    base, table, lookups, out, cnt, rep = case(fname, n, 2, 2, 40, "nonzero", ("zero", None))
    p_words = [(pair.bf.p >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(pair.bf.nlimbs)]          # p itself: the smallest non-canonical value
    V = len(p_words)
    try:
        pl.checked(True)
        for col, row in ((1, 17), (4, 299), (6, 0)):                           # a table column, a looked-up column, a mask column
            call = Call(kind, fname)
            w = pair.base_words(base[col])
            w[V * row:V * (row + 1)] = p_words
            keep = GpuVec.from_numpy(pl, w, pair.base_field)
            call.base_ptrs[col] = keep.ptr
            assert call() == INVALID, call.error()
            msg = call.error()
            assert "canonical" in msg and "ms_lookup_multiplicities" in msg and "d_base" in msg and f"column {col}, row {row};" in msg, msg
            call.unchanged()
        # a column that no tuple names is not read, so it is not scanned: m goes into one that holds all ones
        words = [pair.base_words(c) for c in base]
        words[out][:] = 0xFFFFFFFFFFFFFFFF
        d_base = Matrix([GpuVec.from_numpy(pl, w, pair.base_field) for w in words])
        m, report = lookup_multiplicities(pl, d_base, table, lookups, out=d_base.columns[out])
        check(pair, m, report, cnt, rep, fname)
    finally:
        pl.checked(False)


def test_python_mirror_argument_checks():
    pl, pair = backends.planner("emu"), FIELDS["fp"]
    d_base = upload(pl, pair, [[1, 2], [2, 1], [0, 0]])
    with pytest.raises(MsError) as err:
        lookup_multiplicities(pl, d_base, LookupTuple([0]), [LookupTuple([9])])
    assert err.value.code == INVALID and "out of range" in str(err.value)
    with pytest.raises(MsError) as err:
        lookup_multiplicities(pl, d_base, LookupTuple([0]), [LookupTuple([1])], out=d_base.columns[1])
    assert err.value.code == INVALID and "overlap" in str(err.value)
    with pytest.raises(ValueError):
        lookup_multiplicities(pl, d_base, LookupTuple([0]), [LookupTuple([1, 2])])            # widths differ
    with pytest.raises(ValueError):
        LookupTuple([])
    with pytest.raises(ValueError):
        LookupTuple([0, 1, 2, 3, 4])
    with pytest.raises(ValueError):
        LookupTuple([0], mask=("odd", 1))
    with pytest.raises(ValueError):
        lookup_multiplicities(pl, d_base, LookupTuple([0]), [LookupTuple([1])], out=GpuVec(pl, 3, FP))
    assert (extension.LOOKUP_MAX_WIDTH, extension.LOOKUP_MAX_SETS) == (4, 8)
    m, report = lookup_multiplicities(pl, d_base, LookupTuple([0]), [LookupTuple([1])], out=d_base.columns[2])
    assert m is d_base.columns[2] and report.check() is report and report.first_missing_values() is None
    assert F252F in (f.base_field for f in FIELDS.values())
