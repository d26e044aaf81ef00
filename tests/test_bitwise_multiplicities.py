"""ms_bitwise_multiplicities and ms_bitwise_table (include/ministark_hip_bitwise.h) against the loops on Python integers
(tests/bitwise_ref.py), and against ms_lookup_multiplicities at width 4 on limb columns -- the route they replace -- word for word: a pair
table on each side of every histogram class boundary (bits 6 | 7: 32-bit LDS counters of 16 and 64 KiB; 7 | 8: packed 16-bit counters;
8 | 9: the global form alone) with each counting kernel forced through MS_BITWISE_FORM, both fields, one op and three, limbs that straddle
a 64-bit word, nlimbs * bits = WMAX, sets with and without a result column, a wrong c, an operand at W and 252-bit operands with a high
word set, 64 sets, m in place, a zero tail past the table, the packed counters' flush bounded in increments -- and the refusals, after which
the sentinel-filled d_m and d_report are unchanged.  bits = 11 and 12 are met through validation only: no test holds a 2^24-row table."""
import ctypes

import numpy as np
import pytest

from tests import backends
from tests.bitwise_ref import RANGE_REPORT_FIELDS, apply, bitwise_multiplicities as reference, bitwise_table as table_reference
from tests.test_bitwise_columns import FIELDS, INVALID, KINDS, SENTINEL, UNSUPPORTED, WMAX, below, mask_column, upload, words
from ministark_amd import (BitwiseReport, BitwiseSet, GpuVec, LimbSpec, Matrix, LookupMissing, LookupReport, LookupTuple, bitwise_multiplicities, bitwise_table, extension,
                           limb_decompose, lookup_multiplicities)
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F
from ministark_amd._lib import LookupReportRecord, MsError

FORMS = [None, "plain", "lds"]
AND, OR, XOR = 0, 1, 2


def count_words(fname, counts):
    """the Montgomery words of a long list of small counts: one conversion per distinct count"""
    counts = np.asarray(counts, dtype=np.int64)
    uniq, inv = np.unique(counts, return_inverse=True)
    return np.array([words(fname, [int(u)]) for u in uniq], dtype=np.uint64)[inv].ravel()


def report_dict(report):
    return {k: getattr(report, k) for k in RANGE_REPORT_FIELDS}


def operand_columns(pair, rng, total, n):
    """a, b below W = 2^total, with rows that are NOT in the table: an operand at W, at p - 1, and (Fp252) with a high word set; then
    c_and, c_or, c_xor = a op b with one bit of a few rows flipped"""
    W = 1 << total
    a, b = below(rng, total, n), below(rng, total, n)
    a[0], b[0] = W - 1, W - 1                                                   # the largest pair: in the table
    edges = [(3, W, 1), (5, 1, W), (11, pair.bf.p - 1, 0), (13, W + 1, W - 1)]
    if pair.bf.nlimbs == 4:
        edges += [(17, (1 << 192) + 2, 3), (19, 5, (1 << 128) + (W - 1) % (1 << 64)), (23, (1 << 251) + 1, 1), (29, (1 << 64) % W + (1 << 250), 0)]
    for row, va, vb in edges:
        if row < n:
            a[row], b[row] = va % pair.bf.p, vb % pair.bf.p
    cs = [[apply(op, x, y) % pair.bf.p for x, y in zip(a, b)] for op in (AND, OR, XOR)]
    for op, c in enumerate(cs):
        for row in range(7 + op, n, 97):
            c[row] ^= 1 << ((row + op) % total)                                 # a wrong result: the row is missing, none of its limbs counts
    return [a, b] + cs


def run(kind, fname, base, bits, ops, sets, n_m, what, form=None, monkeypatch=None, in_place=None):
    pl, pair = backends.planner(kind), FIELDS[fname]
    want, rep = reference(base, bits, ops, sets, n_m)
    d = upload(pl, fname, base)
    out = d.columns[in_place] if in_place is not None else GpuVec.from_numpy(pl, np.full(n_m * pair.bf.nlimbs, SENTINEL, dtype=np.uint64), pair.base_field)
    if form is not None:
        monkeypatch.setenv("MS_BITWISE_FORM", form)
    m, report = bitwise_multiplicities(pl, d, bits, ops, sets, out=out, n_m=n_m)
    assert m is out and isinstance(report, BitwiseReport) and isinstance(report, LookupReport)
    got, exp = m.to_numpy()[:n_m * pair.bf.nlimbs], count_words(fname, want)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (what, f"{bad.size} words of m differ, the first is word {int(bad[0])}")
    assert report_dict(report) == rep, what
    for k, (c, v) in enumerate(zip(d.columns, base)):                           # the looked-up columns are only read
        assert k == in_place or np.array_equal(c.to_numpy(), words(fname, v)), what
    return want, rep, report


# (bits, ops): three ops wherever the table stays small; bits = 10 with one op (2^20 rows)
CLASSES = [(1, (AND, OR, XOR)), (4, (XOR,)), (4, (OR, XOR, AND)), (6, (AND, OR, XOR)), (7, (XOR, AND, OR)), (8, (AND,)), (8, (AND, OR, XOR)), (9, (OR, AND, XOR)), (10, (XOR,))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bits,ops", CLASSES, ids=[f"{b}x{len(o)}" for b, o in CLASSES])
def test_every_pair_table_class_in_every_form(kind, fname, form, bits, ops, monkeypatch):
    """one set per op (and a second one without a result column where there is one op), one of each mask kind; n is no multiple of a
    workgroup; n_m is a few rows past the table.  Forcing `lds` on a table that has no LDS form leaves the global one."""
    pair, n = FIELDS[fname], 2500
    nlimbs = min(4, WMAX[fname] // bits)
    rng = np.random.default_rng([bits, n, len(ops)])
    base = operand_columns(pair, rng, nlimbs * bits, n) + [mask_column(rng, n)]
    masks = [("nonzero", 5), None, ("zero", 5)]
    sets = [BitwiseSet(op, 0, 1, 2 + op if s != 1 else None, nlimbs, masks[s]) for s, op in enumerate(ops)]
    if len(ops) == 1:
        sets.append(BitwiseSet(ops[0], 1, 0, None, nlimbs, masks[1]))
    T = len(ops) << (2 * bits)
    want, rep, _ = run(kind, fname, base, bits, ops, sets, T + 5, (fname, form, bits, ops), form, monkeypatch)
    assert rep["missing"] > 20 and sum(want) > n * nlimbs and sum(want) % nlimbs == 0 and want[T:] == [0] * 5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bits,nlimbs", [(6, 11), (7, 10), (9, 8), (10, 7)])
def test_a_limb_that_straddles_two_words(kind, form, bits, nlimbs, monkeypatch):
    """Fp252: the last limb starts below bit 64 and ends above it (bits 60..66, 63..70, 63..72, 60..70); one op keeps the table small"""
    assert (nlimbs - 1) * bits < 64 < nlimbs * bits
    pair, n = FIELDS["fp252"], 700
    rng = np.random.default_rng([bits, nlimbs])
    base = operand_columns(pair, rng, nlimbs * bits, n)
    want, rep, _ = run(kind, "fp252", base, bits, (XOR,), [BitwiseSet(XOR, 0, 1, 4, nlimbs), BitwiseSet(XOR, 1, 0, None, nlimbs)], 1 << (2 * bits), (bits, nlimbs), form, monkeypatch)
    top = ((1 << bits) - 1) << bits | ((1 << bits) - 1)
    assert want[top] >= 2 * nlimbs and rep["missing"] > 8                      # row 0 is (W - 1, W - 1): every limb pair is the last table row


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["plain", "lds"])
@pytest.mark.parametrize("fname,bits,nlimbs", [("fp", 1, 63), ("fp", 7, 9), ("fp", 9, 7), ("fp252", 1, 251)])
def test_limbs_that_fill_the_widest_operand(kind, form, fname, bits, nlimbs, monkeypatch):
    """nlimbs * bits = WMAX exactly: an operand at 2^WMAX is the first value that is out"""
    assert nlimbs * bits == WMAX[fname]
    pair, n = FIELDS[fname], 300
    rng = np.random.default_rng([bits, nlimbs, 1])
    base = operand_columns(pair, rng, nlimbs * bits, n)
    want, rep, _ = run(kind, fname, base, bits, (OR, AND), [BitwiseSet(OR, 0, 1, 3, nlimbs), BitwiseSet(AND, 0, 1, None, nlimbs)], 2 << (2 * bits), (fname, bits), form, monkeypatch)
    assert rep["missing"] > 0 and (rep["first_missing_set"], rep["first_missing_row"]) == (0, 3) and sum(want) % nlimbs == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("form", ["plain", "lds"])
def test_what_is_not_in_the_table_is_missing_and_none_of_its_limbs_counts(kind, fname, form, monkeypatch):
    pair, bits, nlimbs = FIELDS[fname], 4, 2
    W = 1 << (bits * nlimbs)
    for what, (va, vb, vc), values in [("a wrong c", (0x35, 0x5A, 0x35 ^ 0x5A ^ 0x10), None), ("a at W", (W, 1, W ^ 1), None), ("b at p - 1", (1, pair.bf.p - 1, 7), None),
                                       ("no c, a past W", (W + 3, 2, 0), [W + 3, 2, (W + 3) ^ 2])] + \
                                      ([("a high word", ((1 << 192) + 5, 3, ((1 << 192) + 5) ^ 3), None), ("c with a high word", (5, 3, (1 << 64) + (5 ^ 3)), None)] if fname == "fp252" else []):
        a, b, c = [0x12, 0xFF, va, 0x00], [0x34, 0xFF, vb, 0x0F], [0x12 ^ 0x34, 0, vc, 0x0F]
        st = BitwiseSet("xor", 0, 1, None if what.startswith("no c") else 2, nlimbs)
        want, rep, report = run(kind, fname, [a, b, c], bits, (XOR,), [st], 256, (fname, what), form, monkeypatch)
        assert sum(want) == 3 * nlimbs and want[0x13] == 1 and want[0x24] == 1 and want[0xFF] == 2 and want[0x0F] == 1 and want[0x00] == 1
        assert (rep["missing"], rep["first_missing_set"], rep["first_missing_row"]) == (1, 0, 2)
        with pytest.raises(LookupMissing) as err:
            report.check()
        assert (err.value.set, err.value.row, err.value.values, err.value.missing) == (0, 2, values or [va, vb, vc], 1)
        assert "set 0, row 2" in str(err.value) and f"a = {va}, b = {vb}" in str(err.value) and "xor" in str(err.value)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_sixty_four_sets_with_masks(kind, fname):
    pair, n, bits = FIELDS[fname], 257, 5
    rng = np.random.default_rng(64)
    base = operand_columns(pair, rng, 3 * bits, n) + [mask_column(rng, n), mask_column(rng, n)]
    ops = (XOR, AND, OR)
    sets = [BitwiseSet(ops[k % 3], k % 2, 1 - k % 2, [None, 2 + ops[k % 3]][k % 4 != 0], 1 + k % 3, [None, ("nonzero", 5 + k % 2), ("zero", 5 + (k + 1) % 2)][k % 3]) for k in range(64)]
    want, rep, _ = run(kind, fname, base, bits, ops, sets, 3 << (2 * bits), fname)
    assert rep["missing"] > 64 and sum(want) > 64 * n // 3                      # sets of 1 and 2 limbs see 15-bit operands: most of their rows are missing


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_m_may_be_a_column_of_the_trace_that_nothing_names(kind, fname):
    pair, n, bits = FIELDS[fname], 700, 4
    rng = np.random.default_rng(700)
    base = operand_columns(pair, rng, 2 * bits, n) + [mask_column(rng, n), [SENTINEL % pair.bf.p] * n]
    run(kind, fname, base, bits, (AND, XOR), [BitwiseSet(AND, 0, 1, 2, 2, ("nonzero", 5)), BitwiseSet(XOR, 0, 1, 4, 2)], n, fname, in_place=6)   # n_m = n > T = 512: a zero tail


def lds_workgroups(n, incs, bits, nops, cap):
    """ms_bitwise.cpp's lds_grid: the workgroups per op slot of the LDS form"""
    return max(1, min(incs // ((nops * 4) << (2 * bits)), (n + 1023) // 1024, cap // nops))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("fname,nlimbs,nsets", [("fp", 7, 64), ("fp252", 31, 16)])
@pytest.mark.parametrize("shape", ["zero", "alternating"])
def test_the_packed_counters_are_flushed_by_increments_not_rows(kind, form, fname, nlimbs, nsets, shape, monkeypatch):
    """bits = 8, the packed 16-bit counters; 2500 rows of `nsets` sets of `nlimbs` limbs.  The LDS form runs 3 workgroups (1 120 000 or
    1 240 000 increments over 4 * 2^16 is 4; 2500 rows are 3 workgroups of 1024 lanes), so workgroup 0 takes rows 0 .. 1023 of every set:
    1024 * 64 * 7 = 458 752 (Fp) or 1024 * 16 * 31 = 507 904 (Fp252) increments, all of them on bin 0 ("zero": every operand is 0) or half
    on each of the two bins of ONE packed word ("alternating": b's limbs are all 0 or all 1, bins (0, 0) and (0, 1)) -- 229 376 a bin at
    least, against the 65 535 a counter holds.  It takes 64 or 16 rounds of one row a lane: a flush every 63 ROWS would come after 451 584
    increments (Fp) or never (Fp252), and the counters would have wrapped."""
    pl, pair, n, bits = backends.planner(kind), FIELDS[fname], 2500, 8
    assert lds_workgroups(n, n * nsets * nlimbs, bits, 1, 256) == 3 and 1024 * nsets * nlimbs // 2 > 65535
    ones = sum(1 << (bits * j) for j in range(nlimbs))
    a, b = [0] * n, [0 if shape == "zero" or i % 2 == 0 else ones for i in range(n)]
    d = upload(pl, fname, [a, b])
    if form is not None:
        monkeypatch.setenv("MS_BITWISE_FORM", form)
    m, report = bitwise_multiplicities(pl, d, bits, ["or"], [BitwiseSet("or", 0, 1, None, nlimbs)] * nsets, n_m=1 << 16)
    want = np.zeros(1 << 16, dtype=np.int64)
    want[1] = sum(1 for v in b if v) * nsets * nlimbs
    want[0] = n * nsets * nlimbs - want[1]
    assert np.array_equal(m.to_numpy(), count_words(fname, want)) and report_dict(report) == {k: 0 for k in RANGE_REPORT_FIELDS}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("bits,ops,with_op", [(1, (XOR,), False), (3, (OR, XOR), True), (4, (AND, OR, XOR), True), (5, (XOR, AND, OR), False)])
def test_the_table(kind, fname, bits, ops, with_op):
    pl, pair = backends.planner(kind), FIELDS[fname]
    T = len(ops) << (2 * bits)
    for n_t in (T, T + 301):
        out = [GpuVec.from_numpy(pl, np.full((n_t + 2) * pair.bf.nlimbs, SENTINEL, dtype=np.uint64), pair.base_field) if (k or with_op) else None for k in range(4)]
        got = bitwise_table(pl, pair.base_field, bits, ops, n_t=n_t, out=out)
        want = table_reference(bits, ops, n_t)
        for k in range(4):
            if out[k] is None:
                assert got[k] is None
                continue
            w = got[k].to_numpy()
            assert np.array_equal(w[:n_t * pair.bf.nlimbs], words(fname, want[k])) and (w[n_t * pair.bf.nlimbs:] == np.uint64(SENTINEL)).all(), (bits, k)
    new = bitwise_table(pl, pair.base_field, bits, ops)
    assert (new[0] is None) == (len(ops) == 1) and all(len(c) == T for c in new[1:]) and np.array_equal(new[3].to_numpy(), words(fname, table_reference(bits, ops, T)[3]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_it_equals_lookup_multiplicities_on_limb_columns(kind, fname):
    """missing = 0: m equals, word for word, what the hash-table route gives at width 4 over the limb-column tuples (op, a_j, b_j, c_j)
    against bitwise_table's output with n_t = n_m = n; 2 sets of 4 limbs are the 8 lookup sets that route takes"""
    pl, pair, n, bits, nlimbs, ops = backends.planner(kind), FIELDS[fname], 1000, 4, 4, (OR, XOR, AND)
    rng = np.random.default_rng(1000)
    a, b = below(rng, 16, n), below(rng, 16, n)
    a[::3] = [0] * len(a[::3])                                                  # a heavy bin
    zero = [0] * n
    # 0 a, 1 b, 2 c_xor, 3 c_and | 4 op_xor, 5 op_and | 6.. limbs of a, b, c_xor, c_and | 22 top, tx, ty, tz | 26 m
    base = [a, b, [x ^ y for x, y in zip(a, b)], [x & y for x, y in zip(a, b)], [XOR] * n, [AND] * n] + [zero] * 21
    d = upload(pl, fname, base)
    limb_decompose(pl, d, [LimbSpec(src, 6 + 4 * src, nlimbs, bits) for src in range(4)]).check()
    bitwise_table(pl, pair.base_field, bits, ops, n_t=n, out=d.columns[22:26])
    tuples = [LookupTuple([4, 6 + j, 10 + j, 14 + j]) for j in range(nlimbs)] + [LookupTuple([5, 6 + j, 10 + j, 18 + j]) for j in range(nlimbs)]
    m_l, rep_l = lookup_multiplicities(pl, d, LookupTuple([22, 23, 24, 25]), tuples)
    m_b, rep_b = bitwise_multiplicities(pl, d, bits, ops, [BitwiseSet(XOR, 0, 1, 2, nlimbs), BitwiseSet(AND, 0, 1, 3, nlimbs)], out=d.columns[26])
    assert rep_l.missing == 0 and rep_b.missing == 0 and rep_l.duplicate_table_rows == n - 768 and rep_b.duplicate_table_rows == 0
    assert np.array_equal(m_b.to_numpy(), m_l.to_numpy())
    want, _ = reference(base, bits, ops, [BitwiseSet(XOR, 0, 1, 2, nlimbs), BitwiseSet(AND, 0, 1, 3, nlimbs)], n)
    assert np.array_equal(m_b.to_numpy(), count_words(fname, want)) and sum(want[:256]) == 0 and sum(want) == 2 * nlimbs * n


@pytest.mark.gpu
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("bits", [4, 8, 9])
def test_the_result_is_the_same_on_every_run(fname, bits):
    """2^16 rows, three sets over two ops: many workgroups add to the same counters.  Three times in one process: the same words."""
    pl, pair, n, nlimbs = backends.planner("hip"), FIELDS[fname], 1 << 16, 3
    rng = np.random.default_rng([bits, 16])
    a, b = below(rng, nlimbs * bits, n), below(rng, nlimbs * bits, n)
    b[::2] = [0] * (n // 2)
    a[77] = 1 << (nlimbs * bits)
    d = upload(pl, fname, [a, b])
    sets = [BitwiseSet(AND, 0, 1, None, nlimbs), BitwiseSet(XOR, 0, 1, None, nlimbs), BitwiseSet(XOR, 1, 0, None, nlimbs)]
    runs = []
    for _ in range(3):
        m, report = bitwise_multiplicities(pl, d, bits, (XOR, AND), sets, n_m=2 << (2 * bits))
        runs.append((m.to_numpy(), report.buf.to_numpy()))
        assert (report.missing, report.first_missing_set, report.first_missing_row) == (3, 0, 77)
    want, _ = reference([a, b], bits, (XOR, AND), sets, 2 << (2 * bits))
    assert np.array_equal(runs[0][0], count_words(fname, want))
    assert all(np.array_equal(runs[0][0], r[0]) and np.array_equal(runs[0][1], r[1]) for r in runs[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [4, 8])
def test_hot_bins_lose_no_count_at_scale(bits, monkeypatch):
    """2^21 rows, 8 sets of 4 limbs, half of all operands zero: a quarter of the 2^26 limb pairs fall on bin (0, 0) and another half on the
    rows (0, y) and (x, 0), while every workgroup of the LDS form flushes its histogram again and again.  A first build lost a few counts
    in 10^8 here, on some runs (tests/test_bitwise_abi.py has the cause); twice, against numpy."""
    pl, n, nsets, nlimbs = backends.planner("hip"), 1 << 21, 8, 4
    rng = np.random.default_rng([bits, 21])
    lm, eps = np.uint64((1 << bits) - 1), np.uint64(0xFFFFFFFF)                 # x 2^64 = x (2^32 - 1) mod p, below p for x < 2^32
    ab = [rng.integers(0, 1 << (nlimbs * bits), size=n, dtype=np.uint64) for _ in range(2 * nsets)]
    for v in ab:
        v[rng.integers(0, 2, size=n) == 0] = 0
    d = Matrix.from_numpy(pl, [v * eps for v in ab], FP)
    want = np.zeros(1 << (2 * bits), dtype=np.int64)
    for s in range(nsets):
        for j in range(nlimbs):
            sh = np.uint64(bits * j)
            want += np.bincount(((((ab[2 * s] >> sh) & lm) << np.uint64(bits)) | ((ab[2 * s + 1] >> sh) & lm)).astype(np.int64), minlength=want.size)
    assert want[0] > n * nsets * nlimbs // 4 and want.sum() == n * nsets * nlimbs
    monkeypatch.setenv("MS_BITWISE_FORM", "lds")
    for _ in range(2):
        m, report = bitwise_multiplicities(pl, d, bits, ["or"], [BitwiseSet("or", 2 * s, 2 * s + 1, None, nlimbs) for s in range(nsets)], n_m=want.size)
        got = m.to_numpy() // eps
        assert np.array_equal(got.astype(np.int64), want), int(want.sum() - got.astype(np.int64).sum())
        assert report.missing == 0


# ---- refusals and empty cases --------------------------------------------------------------------------------------------------------
class Call:
    """one raw call whose arguments a test can bend: columns 0, 1 operands, 2 a result, 3 a mask, 4 spare; d_m and d_report hold a sentinel"""

    def __init__(self, kind, fname="fp", n=300, bits=3):
        self.pl, self.pair, self.fname = backends.planner(kind), FIELDS[fname], fname
        rng = np.random.default_rng(n)
        self.base = operand_columns(self.pair, rng, 4 * bits, n)[:3] + [mask_column(rng, n), [1] * n]
        self.ops = [AND, XOR]
        self.sets = [[AND, 0, 1, 2, 4, 1, 3, 0], [XOR, 1, 0, -1, 4, 0, 0, 0]]    # op, a, b, c, nlimbs, mask, mask_col, pad
        self.V = self.pair.bf.nlimbs
        self.cols = [GpuVec.from_numpy(self.pl, words(fname, c), self.pair.base_field) for c in self.base]
        self.m = GpuVec.from_numpy(self.pl, np.full(n * self.V, SENTINEL, dtype=np.uint64), self.pair.base_field)
        self.report = GpuVec.from_numpy(self.pl, np.full(4, SENTINEL, dtype=np.uint64), FP)
        self.field, self.n, self.n_m, self.bits, self.nsets, self.nbase, self.nops = self.pair.base_field, n, n, bits, 2, 5, 2
        self.ptrs, self.m_ptr, self.report_ptr, self.null, self.handle = [c.ptr for c in self.cols], self.m.ptr, self.report.ptr, (), self.pl.handle

    def __call__(self):
        rec, ops = np.array(self.sets, dtype=np.int32).reshape(-1, 8), np.array(self.ops, dtype=np.int32)
        arr = None if "base" in self.null else (ctypes.c_void_p * len(self.ptrs))(*self.ptrs)
        return self.pl.lib.ms_bitwise_multiplicities(self.handle, self.field, self.n, arr, self.nbase, self.bits, None if "ops" in self.null else ops.ctypes.data, self.nops,
                                                     None if "sets" in self.null else rec.ctypes.data, self.nsets, self.n_m, self.m_ptr, self.report_ptr)

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self):
        assert (self.m.to_numpy() == np.uint64(SENTINEL)).all() and (self.report.to_numpy() == np.uint64(SENTINEL)).all()

    def record(self):
        rec = LookupReportRecord.from_buffer_copy(self.report.to_numpy().tobytes())
        return {k: int(getattr(rec, k)) for k in RANGE_REPORT_FIELDS}

    def expected(self, n=None):
        mk = lambda r: None if r[5] == 0 else (("nonzero", "zero")[r[5] - 1], r[6])
        sets = [BitwiseSet(r[0], r[1], r[2], None if r[3] < 0 else r[3], r[4], mk(r)) for r in self.sets[:self.nsets]]
        return reference(self.base, self.bits, self.ops[:self.nops], sets, self.n_m, self.n if n is None else n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_the_bent_call_is_accepted_unbent(kind, fname):
    call = Call(kind, fname)
    assert call() == 0, call.error()
    want, rep = call.expected()
    assert np.array_equal(call.m.to_numpy(), count_words(fname, want)) and call.record() == rep and rep["missing"] > 0 and sum(want) > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_null_arguments_limits_indices_and_mask_kinds_are_refused(kind, fname, monkeypatch):
    S = lambda k, w, v: (lambda c: c.sets[k].__setitem__(w, v))
    big = lambda bits: (lambda c: (setattr(c, "bits", bits), [r.__setitem__(4, 1) for r in c.sets]))
    bends = [(lambda c: setattr(c, "handle", None), "null"), (lambda c: setattr(c, "null", ("base",)), "null"), (lambda c: setattr(c, "null", ("sets",)), "null"),
             (lambda c: setattr(c, "null", ("ops",)), "null"), (lambda c: setattr(c, "m_ptr", None), "null"), (lambda c: setattr(c, "report_ptr", None), "null"),
             (lambda c: c.ptrs.__setitem__(4, None), "null base column 4"), (lambda c: setattr(c, "field", 7), ""),
             (lambda c: setattr(c, "bits", 0), "bits"), (lambda c: setattr(c, "bits", 13), "bits"), (lambda c: setattr(c, "nops", 0), "ops"),
             (lambda c: (setattr(c, "nops", 4), setattr(c, "ops", [0, 1, 2, 0])), "ops"), (lambda c: setattr(c, "ops", [XOR, XOR]), "twice"), (lambda c: setattr(c, "ops", [AND, 3]), "unknown op"),
             (lambda c: setattr(c, "n_m", 127), "fewer than the 128 rows"), (big(5), "fewer than the 2048 rows"),
             (big(11), "fewer than the 8388608 rows"),                                            # bits = 11 and 12: validation only
             (lambda c: (big(12)(c), setattr(c, "nops", 1)), "fewer than the 16777216 rows"), (big(12), "table rows (at most 2^24)"),
             (lambda c: setattr(c, "ops", [OR, XOR]), "not one of the table's ops"), (S(1, 0, 5), "unknown op"),
             (S(0, 4, 0), "limbs"), (S(1, 4, 257), "limbs"), (S(0, 4, WMAX[fname] // 3 + 1), "more than the"),
             (S(0, 1, 5), "out of range"), (S(1, 2, -1), "out of range"), (S(0, 3, 5), "out of range"), (S(1, 3, -2), "result column"),
             (S(0, 6, 5), "mask"), (S(0, 6, -1), "mask"), (S(0, 5, 3), "mask kind"), (S(1, 5, -1), "mask kind")]
    for k, (bend, text) in enumerate(bends):
        call = Call(kind, fname)
        bend(call)
        assert call() == INVALID and text in call.error(), (k, call.error())
        call.unchanged()
    monkeypatch.setenv("MS_BITWISE_FORM", "fast")
    call = Call(kind, fname)
    assert call() == INVALID and "MS_BITWISE_FORM" in call.error(), call.error()
    call.unchanged()
    monkeypatch.delenv("MS_BITWISE_FORM")
    call = Call(kind, fname)                                                    # the most limbs the field takes, and n_m = T exactly
    call.sets[0][4], call.n_m = WMAX[fname] // 3, 128
    assert call() == 0, call.error()
    want, rep = call.expected()
    got = call.m.to_numpy()
    assert np.array_equal(got[:128 * call.V], count_words(fname, want)) and (got[128 * call.V:] == np.uint64(SENTINEL)).all() and call.record() == rep


@pytest.mark.parametrize("kind", KINDS)
def test_what_is_too_large_and_fq3_are_unsupported(kind):
    """16 sets of 16 limbs over 2^24 rows are 2^32 limb pairs: refused from the arguments alone -- the columns here hold 300"""
    for bend in (lambda c: (setattr(c, "nsets", 65), setattr(c, "sets", c.sets[:1] * 65)), lambda c: setattr(c, "field", FQ3F),
                 lambda c: (setattr(c, "nsets", 16), setattr(c, "sets", [[AND, 0, 1, 2, 16, 0, 0, 0]] * 16), setattr(c, "n", 1 << 24)),
                 lambda c: (setattr(c, "nsets", 1), setattr(c, "sets", [[AND, 0, 1, 2, 1, 0, 0, 0]]), setattr(c, "n", 1 << 32)), lambda c: setattr(c, "n", (1 << 32) + 1)):
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
    refused(lambda c: setattr(c, "m_ptr", c.ptrs[0]))                            # an operand
    refused(lambda c: setattr(c, "m_ptr", c.ptrs[2]))                            # a result column
    refused(lambda c: setattr(c, "m_ptr", c.ptrs[3]))                            # a mask column
    refused(lambda c: setattr(c, "m_ptr", c.ptrs[1] + col(c) - 8))               # the last word of one
    refused(lambda c: setattr(c, "report_ptr", c.ptrs[2] + 8))
    refused(lambda c: setattr(c, "report_ptr", c.m_ptr))                         # each other
    refused(lambda c: setattr(c, "report_ptr", c.m_ptr + col(c) - 8))
    call = Call(kind, fname)                                                    # the spare column may take m
    call.m_ptr = call.ptrs[4]
    assert call() == 0, call.error()
    want, rep = call.expected()
    assert np.array_equal(call.cols[4].to_numpy(), count_words(fname, want)) and call.record() == rep


@pytest.mark.parametrize("kind", KINDS)
def test_no_rows_and_no_sets(kind):
    for bend in (lambda c: setattr(c, "n", 0), lambda c: (setattr(c, "nsets", 0), setattr(c, "null", ("sets",))), lambda c: (setattr(c, "n", 0), setattr(c, "nsets", 0))):
        call = Call(kind)
        bend(call)
        assert call() == 0, call.error()
        assert (call.m.to_numpy() == 0).all() and call.record() == {k: 0 for k in RANGE_REPORT_FIELDS}


@pytest.mark.parametrize("kind", KINDS)
def test_the_table_refuses_what_the_count_refuses(kind):
    pl = backends.planner(kind)
    cols = [GpuVec.from_numpy(pl, np.full(200, SENTINEL, dtype=np.uint64), FP) for _ in range(4)]
    ops = np.array([AND, XOR, OR, AND], dtype=np.int32)
    call = lambda field=FP, bits=3, nops=2, n_t=200, ptrs=None, h_ops=ops.ctypes.data: pl.lib.ms_bitwise_table(pl.handle, field, bits, h_ops, nops, n_t, *(ptrs or [c.ptr for c in cols]))
    p = [c.ptr for c in cols]
    for kwargs, code, text in [(dict(bits=0), INVALID, "bits"), (dict(bits=13), INVALID, "bits"), (dict(nops=0), INVALID, "ops"), (dict(nops=4), INVALID, "ops"),
                               (dict(n_t=127), INVALID, "fewer than the 128 rows"), (dict(bits=12, nops=1), INVALID, "fewer than the 16777216 rows"), (dict(bits=12), INVALID, "at most 2^24"),
                               (dict(h_ops=None), INVALID, "null"), (dict(ptrs=[p[0], None, p[2], p[3]]), INVALID, "null"), (dict(ptrs=[p[0], p[1], p[1], p[3]]), INVALID, "overlap"),
                               (dict(ptrs=[p[3] + 8, p[1], p[2], p[3]]), INVALID, "overlap"), (dict(field=FQ3F), UNSUPPORTED, "Fq3"),
                               (dict(h_ops=ops[2:].ctypes.data, nops=2), 0, ""), (dict(ptrs=[None] + p[1:], n_t=128), 0, "")]:
        before = [c.to_numpy() for c in cols]
        rc = call(**kwargs)
        assert rc == code and (code == 0 or text in pl.lib.ms_last_error().decode()), (kwargs, pl.lib.ms_last_error().decode())
        assert code == 0 or all(np.array_equal(c.to_numpy(), w) for c, w in zip(cols, before))
    ops4 = np.array([AND, AND], dtype=np.int32)
    assert call(h_ops=ops4.ctypes.data) == INVALID and "twice" in pl.lib.ms_last_error().decode()


@pytest.mark.parametrize("kind", KINDS)
def test_checked_mode_names_column_and_row(kind):
    pl = backends.planner(kind)
    try:
        pl.checked(True)
        for col, row in ((0, 17), (1, 299), (2, 0), (3, 150)):
            call = Call(kind)
            w = words("fp", call.base[col])
            w[row] = FIELDS["fp"].bf.p
            keep = GpuVec.from_numpy(pl, w, FP)
            call.ptrs[col] = keep.ptr
            assert call() == INVALID, call.error()
            msg = call.error()
            assert "canonical" in msg and "ms_bitwise_multiplicities" in msg and f"column {col}, row {row};" in msg, msg
            call.unchanged()
        call = Call(kind)                                                       # a column that no set names is not scanned, and may take m
        bad = GpuVec.from_numpy(pl, np.full(call.n, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), FP)
        call.ptrs[4] = call.m_ptr = bad.ptr
        assert call() == 0, call.error()
        want, rep = call.expected()
        assert np.array_equal(bad.to_numpy(), count_words("fp", want)) and call.record() == rep
    finally:
        pl.checked(False)


def test_python_mirror_argument_checks():
    pl = backends.planner("emu")
    d = upload(pl, "fp", [[3, 0, 3, 4, 1], [1, 0, 2, 0, 3], [2, 0, 1, 4, 3]])
    m, report = bitwise_multiplicities(pl, d, 2, ["xor"], [BitwiseSet("xor", 0, 1, 2, 1)], n_m=16)
    assert len(m) == 16 and [int(x != 0) for x in m.to_numpy()] == [1 if j in (0b1101, 0b0000, 0b1110) else 0 for j in range(16)] and not report
    assert (report.missing, report.first_missing_set, report.first_missing_row, report.first_missing_values()) == (2, 0, 3, [4, 0, 4])
    m, report = bitwise_multiplicities(pl, d, 2, ["xor"], [], n_m=16)
    assert list(m.to_numpy()) == [0] * 16 and report.check() is report
    with pytest.raises(MsError) as err:
        bitwise_multiplicities(pl, d, 2, ["xor"], [BitwiseSet("xor", 0, 3, None, 1)], n_m=16)
    assert err.value.code == INVALID and "out of range" in str(err.value)
    with pytest.raises(MsError) as err:
        bitwise_multiplicities(pl, d, 2, ["xor"], [BitwiseSet("xor", 0, 1, None, 1)], out=GpuVec(pl, 16, FP).__class__.from_numpy(pl, np.zeros(16, dtype=np.uint64), FP), n_m=16) if False else bitwise_multiplicities(pl, d, 1, ["xor"], [BitwiseSet("xor", 0, 1, None, 1)], out=d.columns[0])
    assert err.value.code == INVALID and "overlap" in str(err.value)
    B = lambda **kw: bitwise_multiplicities(pl, d, kw.pop("bits", 2), kw.pop("ops", ["xor"]), kw.pop("sets", [BitwiseSet("xor", 0, 1, None, 1)]), **{"n_m": 16, **kw})
    assert B()[1].missing == 1
    for bad in (lambda: B(bits=0), lambda: B(bits=13), lambda: B(bits=3, n_m=63), lambda: B(ops=[]), lambda: B(ops=["xor", "xor"]), lambda: B(ops=["and"]), lambda: B(ops=["nor"]),
                lambda: B(sets=[BitwiseSet("xor", 0, 1, None, 32)]), lambda: B(sets=[BitwiseSet("xor", 0, 1, None, 1)] * 65), lambda: B(n_m=15),
                lambda: B(out=GpuVec(pl, 16, FP), n_m=17), lambda: BitwiseSet("xor", 0, 1, -1, 1), lambda: BitwiseSet("xor", 0, 1, None, 0), lambda: BitwiseSet("xor", 0, 1, None, 257),
                lambda: bitwise_table(pl, FP, 2, ["xor"], n_t=15), lambda: bitwise_table(pl, FQ3F, 2, ["xor"]), lambda: bitwise_table(pl, FP, 12, ["xor", "and"])):
        with pytest.raises(ValueError):
            bad()
    assert (extension.BITWISE_MAX_SETS, extension.BITWISE_MAX_BITS, extension.BITWISE_MAX_LIMBS) == (64, 12, 256)
