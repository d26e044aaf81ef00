"""ms_join_rows (include/ministark_hip_join.h) against the loop on Python integers (tests/join_ref.py), match arrays and report word for
word: table and probe lengths crossed (table shorter than, as long as, longer than the rows joined), widths 1..4, both fields, 1..3 sets,
the three masks on either side, tables so small that the probe walk wraps, keys that differ in one word only (every component, every
limb), the all-equal table, the all-inactive table, every row hitting one table row, the sequential-key table, missing keys in several
sets, the self-join, zero sizes, `fetch_columns` -- and the refusals, after which the sentinel-filled d_match and d_report are unchanged.
What only the device can show -- that the build's races leave the smallest row in the slot, and a lane's second row past the grid cap --
is the `hip` half of every case, the case past the cap and the determinism test."""
import ctypes
import functools

import numpy as np
import pytest

from tests import backends
from tests.ext_ref import PAIRS
from tests.join_ref import NONE, REPORT_FIELDS, first_rows, reference
from ministark_amd import DeviceIndex, GpuVec, JoinReport, LookupMissing, LookupTuple, Matrix, extension, fetch_columns, join_rows
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F
from ministark_amd._lib import JoinReportRecord, MsError

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = {"fp": PAIRS["fp_fp"], "fp252": PAIRS["fp252_fp252"]}
TABLE_LENGTHS = [1, 2, 3, 255, 256, 257, 1000]
LENGTHS = [1, 2, 257, 1025, 4097]
INVALID, UNSUPPORTED = -1, -2
SENTINEL = 0xA5A5A5A5A5A5A5A5
MASKS = [None, "nonzero", "zero"]


def rand_values(pair, rng, count):
    if pair.bf.nlimbs == 1:
        return [int(v) for v in rng.integers(0, pair.bf.p, size=count, dtype=np.uint64)]
    return [int.from_bytes(rng.bytes(32), "little") % pair.bf.p for _ in range(count)]


def layout(width, nsets, table_mask=None, key_masks=None):
    """table columns: the key's `width`, two mask columns, one payload column.  base columns: every set's `width`, then two mask columns.
    -> (table_key, keys, ntable_cols, nbase)"""
    mk = lambda kind, col: None if kind is None else (kind, col)
    table_key = LookupTuple(range(width), mk(table_mask, width))
    mask_a, mask_b = width * nsets, width * nsets + 1
    keys = [LookupTuple(range(width * s, width * (s + 1)), mk((key_masks or [None] * nsets)[s], mask_b if s % 2 == 0 else mask_a)) for s in range(nsets)]
    return table_key, keys, width + 3, width * nsets + 2


def mask_column(rng, n):
    return [int(v) if k else 0 for v, k in zip(rng.integers(1, 1 << 62, size=n), rng.integers(0, 3, size=n))]


@functools.lru_cache(maxsize=None)
def case(fname, n_table, n, width, nsets, npool, table_mask=None, key_masks=None, seed=0):
    """(table columns, base columns as integers, table_key, keys, expected matches, expected report), computed once and shared by the
    backends.  The table's rows are drawn from a pool of `npool` keys (npool < n_table: equal rows); a joined row is drawn from the pool and
    from an eighth as many foreign keys again, so the pool's keys that the table happens not to hold, and every foreign one, are missing."""
    pair = FIELDS[fname]
    rng = np.random.default_rng([n_table, n, width, nsets, npool, seed])
    table_key, keys, ntc, nbase = layout(width, nsets, table_mask, key_masks)
    vals = rand_values(pair, rng, 2 * npool * width)
    pool = [tuple(vals[k * width:(k + 1) * width]) for k in range(2 * npool)]
    table = [[0] * n_table for _ in range(ntc)]
    for j, k in enumerate(rng.integers(0, npool, size=n_table)):
        for c in range(width):
            table[c][j] = pool[k][c]
    table[width], table[width + 1] = mask_column(rng, n_table), mask_column(rng, n_table)
    table[width + 2] = rand_values(pair, rng, n_table)
    base = [[0] * n for _ in range(nbase)]
    for s in range(nsets):
        for i, k in enumerate(rng.integers(0, npool + max(1, npool // 8), size=n)):
            for c in range(width):
                base[width * s + c][i] = pool[k][c]
    base[nbase - 2], base[nbase - 1] = mask_column(rng, n), mask_column(rng, n)
    match, rep = reference(table, table_key, base, keys)
    return table, base, table_key, keys, match, rep


def upload(pl, pair, cols):
    return Matrix([GpuVec.from_numpy(pl, pair.base_words(c), pair.base_field) for c in cols])


def report_dict(report):
    return {k: getattr(report, k) for k in REPORT_FIELDS}


def check(matches, report, match, rep, what):
    assert len(matches) == len(match), what
    for s, (got, want) in enumerate(zip(matches, match)):
        got, want = got.to_numpy(), np.array(want, dtype=np.uint32)
        bad = np.nonzero(got != want)[0]
        assert got.dtype == np.uint32 and got.size == want.size and bad.size == 0, (what, f"set {s}: {bad.size} entries differ, the first in row {int(bad[0]) if bad.size else -1}")
    assert report_dict(report) == rep, what


def run_join(kind, fname, table, table_key, base, keys, match, rep, what):
    pl, pair = backends.planner(kind), FIELDS[fname]
    d_table, d_base = upload(pl, pair, table), upload(pl, pair, base)
    matches, report = join_rows(pl, d_table, table_key, d_base, keys)
    check(matches, report, match, rep, what)
    for d, host in ((d_table, table), (d_base, base)):                         # both sides are only read
        for c, v in zip(d.columns, host):
            assert np.array_equal(c.to_numpy(), pair.base_words(v)), what
    return matches, report


def run_case(kind, fname, *args, **kw):
    table, base, table_key, keys, match, rep = case(fname, *args, **kw)
    run_join(kind, fname, table, table_key, base, keys, match, rep, (fname, args, kw))
    return rep


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("n_table", TABLE_LENGTHS)
def test_table_and_probe_lengths_crossed(kind, fname, n_table, n):
    """every table length against every probe length at every width; the number of sets and the masks of both sides go round with the width"""
    for width in (1, 2, 3, 4):
        nsets = 1 + width % 3
        shift = TABLE_LENGTHS.index(n_table) + LENGTHS.index(n)
        run_case(kind, fname, n_table, n, width, nsets, max(1, n_table // 2), MASKS[(width + shift) % 3], tuple(MASKS[(width + shift + 1 + s) % 3] for s in range(nsets)))


@pytest.mark.parametrize("kind", KINDS)
def test_two_hundred_tables_of_at_most_eight_rows(kind):
    """capacities 2 .. 16: the probe walk wraps round the end of the slot array"""
    rng = np.random.default_rng(8)
    seen_missing = seen_dups = 0
    for k in range(200):
        fname = ("fp", "fp252")[k % 2]
        n_table, n, width, nsets = int(rng.integers(1, 9)), int(rng.integers(1, 20)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
        table_key, keys, ntc, nbase = layout(width, nsets, MASKS[k % 3] if k % 5 == 0 else None, [MASKS[(k + s) % 3] if k % 7 == 0 else None for s in range(nsets)])
        table = [[int(v) for v in rng.integers(0, 3, size=n_table)] for _ in range(ntc)]          # values 0, 1, 2: every kind of coincidence
        base = [[int(v) for v in rng.integers(0, 3, size=n)] for _ in range(nbase)]
        match, rep = reference(table, table_key, base, keys)
        run_join(kind, fname, table, table_key, base, keys, match, rep, (k, fname, table, base))
        seen_missing += rep["missing"] > 0
        seen_dups += rep["duplicate_table_rows"] > 0
    assert seen_missing > 20 and seen_dups > 20


def limbs_to_words(residues, nlimbs):
    return np.array([(r >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for r in residues for k in range(nlimbs)], dtype=np.uint64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_keys_that_differ_in_one_word_only(kind, fname, width):
    """Residues are uploaded as they are (all below p, so canonical): row 0 of the table is a key K, row 1 + v the same key with one bit of
    ONE word flipped -- every component, every limb.  A compare or a hash that skips that word takes the row for row 0: every variant is
    joined several times, in a shuffled order, and has to come back with its own row."""
    pl, pair = backends.planner(kind), FIELDS[fname]
    L = pair.bf.nlimbs
    rng = np.random.default_rng(width)
    K = [int.from_bytes(rng.bytes(8 * L - 2), "little") for _ in range(width)]                # below 2^(64 L - 16) < p
    rows = [tuple(K)] + [tuple(x ^ (1 << (64 * l + 7)) if c == cc else x for cc, x in enumerate(K)) for c in range(width) for l in range(L)]
    assert len(set(rows)) == 1 + width * L and all(x < pair.bf.p for r in rows for x in r)
    order = rng.permutation(3 * len(rows)) % len(rows)
    table = [[r[c] for r in rows] for c in range(width)]
    base = [[rows[k][c] for k in order] for c in range(width)]
    table_key, keys = LookupTuple(range(width)), [LookupTuple(range(width))]
    match, rep = reference(table, table_key, base, keys)
    assert match[0] == [int(k) for k in order] and rep["missing"] == 0 and rep["duplicate_table_rows"] == 0
    d_table = Matrix([GpuVec.from_numpy(pl, limbs_to_words(c, L), pair.base_field) for c in table])
    d_base = Matrix([GpuVec.from_numpy(pl, limbs_to_words(c, L), pair.base_field) for c in base])
    matches, report = join_rows(pl, d_table, table_key, d_base, keys)
    check(matches, report, match, rep, (fname, width))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_a_table_whose_rows_are_all_equal(kind, fname):
    """every insert meets the same slot; row 0 is every match and the other rows are duplicates"""
    n_table, n = 1024, 700
    table = [[7] * n_table, [9] * n_table]
    base = [[7] * (n - 3) + [8] * 3, [9] * n]
    table_key, keys = LookupTuple([0, 1]), [LookupTuple([0, 1])]
    match, rep = reference(table, table_key, base, keys)
    assert match == [[0] * (n - 3) + [NONE] * 3]
    assert rep == {"matched": n - 3, "missing": 3, "first_missing_set": 0, "first_missing_row": n - 3, "duplicate_table_rows": n_table - 1, "table_active": n_table}
    run_join(kind, fname, table, table_key, base, keys, match, rep, fname)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_a_table_whose_rows_are_all_inactive(kind, fname):
    n_table, n = 300, 400
    rng = np.random.default_rng(300)
    table = [[int(v) for v in rng.integers(0, 50, size=n_table)], [0] * n_table]
    base = [[int(v) for v in rng.integers(0, 50, size=n)], [int(v) for v in rng.integers(0, 2, size=n)]]
    table_key, keys = LookupTuple([0], ("nonzero", 1)), [LookupTuple([0], ("zero", 1))]
    match, rep = reference(table, table_key, base, keys)
    nact = base[1].count(0)
    assert match == [[NONE] * n] and rep == {"matched": 0, "missing": nact, "first_missing_set": 0, "first_missing_row": base[1].index(0), "duplicate_table_rows": 0, "table_active": 0}
    run_join(kind, fname, table, table_key, base, keys, match, rep, fname)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_every_row_hits_one_table_row(kind, fname):
    pair = FIELDS[fname]
    n_table, n, hot = 1000, 4097, 777
    rng = np.random.default_rng(17)
    t = rand_values(pair, rng, n_table)
    assert len(set(t)) == n_table
    table, base = [t], [[t[hot]] * n]
    table_key, keys = LookupTuple([0]), [LookupTuple([0])]
    match, rep = reference(table, table_key, base, keys)
    assert match == [[hot] * n] and rep["matched"] == n and rep["missing"] == 0
    run_join(kind, fname, table, table_key, base, keys, match, rep, fname)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_the_sequential_key_table(kind, fname):
    """keys 0 .. n_table - 1: sequential multiples of one constant in Montgomery form"""
    n_table, n = 4096, 3000
    rng = np.random.default_rng(n_table)
    table, base = [list(range(n_table))], [[int(v) for v in rng.integers(0, n_table + 50, size=n)]]
    table_key, keys = LookupTuple([0]), [LookupTuple([0])]
    match, rep = reference(table, table_key, base, keys)
    assert match[0] == [v if v < n_table else NONE for v in base[0]] and rep["missing"] > 0 and rep["duplicate_table_rows"] == 0
    run_join(kind, fname, table, table_key, base, keys, match, rep, fname)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_missing_keys_in_several_sets(kind, fname):
    pl, pair = backends.planner(kind), FIELDS[fname]
    n_table, n = 200, 600
    rng = np.random.default_rng(600)
    t = [rand_values(pair, rng, n_table) for _ in range(2)]
    sets = []
    for s in range(3):
        idx = rng.integers(0, n_table, size=n)
        sets.append([[t[0][j] for j in idx], [t[1][j] for j in idx]])
    # the first component of a pair alone is in the table, the second alone too: the pair is not
    for s, i in ((1, 599), (1, 258), (2, 0), (2, 300), (1, 257)):
        sets[s][1][i] = t[1][(t[0].index(sets[s][0][i]) + 1) % n_table]
    base = [c for st in sets for c in st]
    table_key, keys = LookupTuple([0, 1]), [LookupTuple([0, 1]), LookupTuple([2, 3]), LookupTuple([4, 5])]
    match, rep = reference(t, table_key, base, keys)
    assert rep == {"matched": 3 * n - 5, "missing": 5, "first_missing_set": 1, "first_missing_row": 257, "duplicate_table_rows": 0, "table_active": n_table}
    matches, report = run_join(kind, fname, t, table_key, base, keys, match, rep, fname)
    assert isinstance(report, JoinReport) and not report and "missing=5" in repr(report)
    assert report.first_missing_values() == [base[2][257], base[3][257]]
    with pytest.raises(LookupMissing) as err:
        report.check()
    assert (err.value.set, err.value.row, err.value.values, err.value.missing) == (1, 257, [base[2][257], base[3][257]], 5)
    assert "set 1, row 257" in str(err.value)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_a_self_join(kind, fname):
    """d_table is d_base: a row's own key is in the table, held by itself or by an earlier row"""
    pl, pair = backends.planner(kind), FIELDS[fname]
    n = 1025
    rng = np.random.default_rng(1025)
    cols = [[int(v) for v in rng.integers(0, 300, size=n)], [int(v) for v in rng.integers(0, 2, size=n)], mask_column(rng, n)]
    key, masked = LookupTuple([0, 1]), LookupTuple([0, 1], ("nonzero", 2))
    match, rep = reference(cols, key, cols, [key, masked])
    assert all(m <= i for i, m in enumerate(match[0])) and rep["missing"] == 0 and rep["duplicate_table_rows"] > 0
    assert any(m < i for i, m in enumerate(match[0])) and NONE in match[1]
    d = upload(pl, pair, cols)
    matches, report = join_rows(pl, d, key, d, [key, masked])
    check(matches, report, match, rep, fname)
    match, rep = reference(cols, masked, cols, [key])                           # the masked table: rows whose key only an inactive row holds are missing
    assert rep["missing"] > 0 and rep["table_active"] < n
    matches, report = join_rows(pl, d, masked, d, [key])
    check(matches, report, match, rep, fname)
    for c, v in zip(d.columns, cols):
        assert np.array_equal(c.to_numpy(), pair.base_words(v))


@pytest.mark.gpu
def test_a_lane_takes_a_second_row_past_the_grid_cap():
    """4096 workgroups of 256 lanes is the most stream_grid gives: with 2^20 + 257 rows the first 257 lanes take a second row"""
    pl, pair = backends.planner("hip"), FIELDS["fp"]
    n_table, n = 1000, (1 << 20) + 257
    rng = np.random.default_rng(20)
    pool = np.unique(rng.integers(0, pair.bf.p, size=2 * n_table, dtype=np.uint64))[:n_table + 100]
    rng.shuffle(pool)
    words = np.array(pair.base_words([int(v) for v in pool]), dtype=np.uint64)
    pick = rng.integers(0, n_table + 100, size=n)
    pick[-257:] = np.arange(257) * 4 % (n_table + 100)                        # the rows of the second round: matches and misses
    want = np.where(pick < n_table, pick, NONE).astype(np.uint32)
    d_table, d_base = Matrix([GpuVec.from_numpy(pl, words[:n_table], FP)]), Matrix([GpuVec.from_numpy(pl, words[pick], FP)])
    (match,), report = join_rows(pl, d_table, LookupTuple([0]), d_base, [LookupTuple([0])])
    got = match.to_numpy()
    assert np.array_equal(got, want), int(np.nonzero(got != want)[0][0])
    nmiss = int((want == NONE).sum())
    assert report_dict(report) == {"matched": n - nmiss, "missing": nmiss, "first_missing_set": 0, "first_missing_row": int(np.nonzero(want == NONE)[0][0]),
                                   "duplicate_table_rows": 0, "table_active": n_table}


@pytest.mark.gpu
@pytest.mark.parametrize("fname", list(FIELDS))
def test_the_result_is_the_same_on_every_run(fname):
    """a table of 4097 rows drawn from 64 keys, three sets: the inserts race for the same slots.  Three times in one process: the same match
    arrays, the same report, and all the reference's."""
    pl, pair = backends.planner("hip"), FIELDS[fname]
    table, base, table_key, keys, match, rep = case(fname, 4097, 4097, 2, 3, 64, None, (None, "nonzero", "zero"))
    assert rep["duplicate_table_rows"] >= 4097 - 64 and rep["missing"] > 100
    d_table, d_base = upload(pl, pair, table), upload(pl, pair, base)
    runs = []
    for _ in range(3):
        matches, report = join_rows(pl, d_table, table_key, d_base, keys)
        check(matches, report, match, rep, fname)
        runs.append(([m.to_numpy() for m in matches], report.buf.to_numpy()))
    assert all(np.array_equal(runs[0][1], r[1]) and all(np.array_equal(a, b) for a, b in zip(runs[0][0], r[0])) for r in runs[1:])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_fetch_columns_against_the_payload_of_the_first_row(kind, fname):
    pl, pair = backends.planner(kind), FIELDS[fname]
    table, base, table_key, keys, match, rep = case(fname, 257, 1025, 2, 1, 100, "nonzero", ("zero",))
    first, _, _ = first_rows(table, table_key, 257)
    assert rep["missing"] > 0 and NONE in match[0]
    payload = [4, 0]                                                            # the payload column and a key column
    want = [[table[c][j] if j != NONE else 0 for j in match[0]] for c in payload]
    assert all(want[0][i] == table[4][first[(base[0][i], base[1][i])]] for i in range(1025) if match[0][i] != NONE)
    d_table, d_base = upload(pl, pair, table), upload(pl, pair, base)
    fetched, report = fetch_columns(pl, d_table, table_key, d_base, keys[0], payload)
    assert report_dict(report) == rep
    for got, w in zip(fetched.columns, want):
        assert np.array_equal(got.to_numpy(), pair.base_words(w))               # unmatched and inactive rows: zero elements
    outs = [GpuVec.from_numpy(pl, np.full(1025 * pair.bf.nlimbs, SENTINEL, dtype=np.uint64), pair.base_field) for _ in payload]
    fetched, report = fetch_columns(pl, d_table, table_key, d_base, keys[0], payload, out=outs)
    assert all(a is b for a, b in zip(fetched.columns, outs))
    for got, w in zip(outs, want):
        assert np.array_equal(got.to_numpy(), pair.base_words(w))
    with pytest.raises(LookupMissing) as err:
        fetch_columns(pl, d_table, table_key, d_base, keys[0], payload, check=True)
    assert (err.value.set, err.value.row, err.value.missing) == (0, rep["first_missing_row"], rep["missing"])
    with pytest.raises(ValueError):
        fetch_columns(pl, d_table, table_key, d_base, keys[0], [5])
    with pytest.raises(ValueError):
        fetch_columns(pl, d_table, table_key, d_base, keys[0], [])


# ---- refusals and empty cases --------------------------------------------------------------------------------------------------------
class Call:
    """one raw call whose arguments a test can bend; every d_match and d_report are filled with a sentinel"""

    def __init__(self, kind, fname="fp", n_table=120, n=300):
        self.pl, self.pair = backends.planner(kind), FIELDS[fname]
        table, base, table_key, keys, self.want, self.rep = case(fname, n_table, n, 2, 2, 40, "nonzero", ("zero", None))
        self.d_table, self.d_base = upload(self.pl, self.pair, table), upload(self.pl, self.pair, base)
        self.field, self.n_table, self.n, self.width, self.nsets = self.pair.base_field, n_table, n, 2, 2
        self.table_ptrs, self.base_ptrs = [c.ptr for c in self.d_table.columns], [c.ptr for c in self.d_base.columns]
        self.table_key, self.keys = table_key._record(), [k._record() for k in keys]
        self.V = self.pair.bf.nlimbs
        self.match = [GpuVec.from_numpy(self.pl, np.full((n + 1) // 2, SENTINEL, dtype=np.uint64), FP) for _ in range(8)]
        self.report = GpuVec.from_numpy(self.pl, np.full(6, SENTINEL, dtype=np.uint64), FP)
        self.match_ptrs, self.report_ptr, self.null, self.handle = [m.ptr for m in self.match], self.report.ptr, (), self.pl.handle

    def __call__(self):
        trec = np.array(self.table_key, dtype=np.int32)
        krec = np.array(self.keys, dtype=np.int32).reshape(-1, 8)
        VP = ctypes.c_void_p
        arr = lambda name, ptrs: None if name in self.null else (VP * max(1, len(ptrs)))(*ptrs)
        return self.pl.lib.ms_join_rows(self.handle, self.field, self.n_table, arr("table", self.table_ptrs), len(self.table_ptrs),
                                        None if "table_key" in self.null else trec.ctypes.data, self.n, arr("base", self.base_ptrs), len(self.base_ptrs), self.width,
                                        None if "keys" in self.null else krec.ctypes.data, self.nsets, arr("match", self.match_ptrs[:max(1, self.nsets)]), self.report_ptr)

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self):
        assert all((m.to_numpy() == np.uint64(SENTINEL)).all() for m in self.match) and (self.report.to_numpy() == np.uint64(SENTINEL)).all()

    def matches(self, s, n=None):
        return self.match[s].to_numpy().view(np.uint32)[:self.n if n is None else n]

    def record(self):
        rec = JoinReportRecord.from_buffer_copy(self.report.to_numpy().tobytes())
        return {k: int(getattr(rec, k)) for k in REPORT_FIELDS}


@pytest.mark.parametrize("kind", KINDS)
def test_the_bent_call_is_accepted_unbent(kind):
    call = Call(kind)
    assert call() == 0, call.error()
    assert all(np.array_equal(call.matches(s), np.array(call.want[s], dtype=np.uint32)) for s in range(2)) and call.record() == call.rep
    assert all((m.to_numpy() == np.uint64(SENTINEL)).all() for m in call.match[2:])


@pytest.mark.parametrize("kind", KINDS)
def test_null_arguments_widths_indices_and_mask_kinds_are_refused(kind):
    ntable_cols, nbase = 5, 6
    bends = [lambda c: setattr(c, "handle", None), lambda c: setattr(c, "null", ("table",)), lambda c: setattr(c, "null", ("table_key",)),
             lambda c: setattr(c, "null", ("base",)), lambda c: setattr(c, "null", ("keys",)), lambda c: setattr(c, "null", ("match",)),
             lambda c: setattr(c, "report_ptr", None), lambda c: c.match_ptrs.__setitem__(1, None),
             lambda c: c.table_ptrs.__setitem__(4, None), lambda c: c.base_ptrs.__setitem__(5, None), lambda c: setattr(c, "field", 7),
             lambda c: setattr(c, "width", 0), lambda c: setattr(c, "width", 5),
             lambda c: c.table_key.__setitem__(1, ntable_cols), lambda c: c.table_key.__setitem__(0, -1),                                    # a table column
             lambda c: c.keys[1].__setitem__(0, nbase), lambda c: c.keys[0].__setitem__(1, -1),                                              # a base column
             lambda c: c.table_key.__setitem__(5, ntable_cols), lambda c: c.keys[0].__setitem__(5, -1),                                      # a mask column
             lambda c: c.table_key.__setitem__(4, 3), lambda c: c.keys[0].__setitem__(4, -1)]                                                # a mask kind
    for k, bend in enumerate(bends):
        call = Call(kind)
        assert (len(call.table_ptrs), len(call.base_ptrs)) == (ntable_cols, nbase)
        bend(call)
        assert call() == INVALID, (k, call.error())
        call.unchanged()
    # which side and which set: a base index that the table would hold, a table index that the base would hold
    call = Call(kind)
    call.keys[1][0] = nbase
    assert call() == INVALID and "d_base" in call.error() and "set 1" in call.error() and "out of range" in call.error(), call.error()
    call = Call(kind)
    call.table_key[0] = ntable_cols                                             # 5: a column of d_base, not of d_table
    assert call() == INVALID and "d_table" in call.error() and "out of range" in call.error(), call.error()
    call = Call(kind)
    call.keys[0][5] = nbase
    assert call() == INVALID and "d_base" in call.error() and "set 0" in call.error() and "mask" in call.error(), call.error()
    call = Call(kind)                                                           # what is not read is not checked: the components past the width, an unmasked key's mask column
    call.table_key[2], call.table_key[3], call.keys[1][5] = 99, -7, 99
    assert call() == 0, call.error()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_overlapping_outputs_are_refused(kind, fname):
    def refused(bend):
        call = Call(kind, fname)
        bend(call)
        assert call() == INVALID and "overlap" in call.error(), call.error()
        call.unchanged()
    tcol, col, mbytes = (lambda c: 8 * c.V * c.n_table), (lambda c: 8 * c.V * c.n), (lambda c: 4 * c.n)
    refused(lambda c: c.match_ptrs.__setitem__(0, c.table_ptrs[0]))                              # a key column of the table
    refused(lambda c: c.match_ptrs.__setitem__(1, c.table_ptrs[2]))                              # the table's mask column
    refused(lambda c: c.match_ptrs.__setitem__(1, c.table_ptrs[1] + tcol(c) - 8))                # the last word of one
    refused(lambda c: c.match_ptrs.__setitem__(0, c.base_ptrs[3]))                               # a key column of the other set
    refused(lambda c: c.match_ptrs.__setitem__(1, c.base_ptrs[5]))                               # a mask column of the base
    refused(lambda c: c.match_ptrs.__setitem__(0, c.base_ptrs[0] + col(c) - 4))
    refused(lambda c: setattr(c, "report_ptr", c.table_ptrs[1] + 8))
    refused(lambda c: setattr(c, "report_ptr", c.base_ptrs[2] + col(c) - 8))
    refused(lambda c: c.match_ptrs.__setitem__(1, c.match_ptrs[0]))                              # each other
    refused(lambda c: c.match_ptrs.__setitem__(1, c.match_ptrs[0] + mbytes(c) - 4))
    refused(lambda c: setattr(c, "report_ptr", c.match_ptrs[1]))
    refused(lambda c: setattr(c, "report_ptr", c.match_ptrs[0] + mbytes(c) - 4))
    call = Call(kind, fname)                                                    # columns that no key and no mask names may take an output
    assert call.table_key[5] == 2 and call.keys[0][5] == 5 and call.keys[1][4] == 0
    if call.V * 8 * call.n_table >= 4 * call.n:
        call.match_ptrs[0] = call.table_ptrs[3]                                 # the table's second mask column
    call.report_ptr = call.table_ptrs[4]                                        # its payload column
    call.match_ptrs[1] = call.base_ptrs[4]                                      # the base's first mask column
    assert call() == 0, call.error()


@pytest.mark.parametrize("kind", KINDS)
def test_what_is_too_large_and_fq3_are_unsupported(kind):
    for bend in (lambda c: (setattr(c, "nsets", 9), setattr(c, "keys", c.keys[:1] * 9), setattr(c, "match_ptrs", c.match_ptrs + c.match_ptrs[:1])),
                 lambda c: setattr(c, "field", FQ3F), lambda c: setattr(c, "n_table", (1 << 30) + 1), lambda c: setattr(c, "n", (1 << 32) + 1)):
        call = Call(kind)
        bend(call)
        assert call() == UNSUPPORTED, call.error()
        call.unchanged()
    call = Call(kind)                                                           # eight sets are accepted
    call.nsets, call.keys = 8, call.keys * 4
    assert call() == 0, call.error()
    assert all(np.array_equal(call.matches(s), np.array(call.want[s % 2], dtype=np.uint32)) for s in range(8))
    assert call.record()["matched"] == 4 * call.rep["matched"] and call.record()["missing"] == 4 * call.rep["missing"]


@pytest.mark.parametrize("kind", KINDS)
def test_no_table_rows_no_rows_and_no_sets(kind):
    table, base, table_key, keys, _, _ = case("fp", 120, 300, 2, 2, 40, "nonzero", ("zero", None))
    call = Call(kind)                                                           # an empty table: every active row is missing
    call.n_table = 0
    assert call() == 0, call.error()
    match, rep = reference(table, table_key, base, keys, n_table=0)
    assert rep["matched"] == 0 and rep["missing"] > 300 and rep["table_active"] == 0
    assert all((call.matches(s) == NONE).all() for s in range(2)) and call.record() == rep
    call = Call(kind)                                                           # no rows: the table is still counted
    call.n = 0
    assert call() == 0, call.error()
    match, rep = reference(table, table_key, base, keys, n=0)
    assert rep["table_active"] > 0 and rep["duplicate_table_rows"] > 0 and rep["matched"] == rep["missing"] == 0
    assert all((m.to_numpy() == np.uint64(SENTINEL)).all() for m in call.match) and call.record() == rep
    call = Call(kind)                                                           # no sets: only the report
    call.nsets, call.null = 0, ("keys", "match")
    assert call() == 0, call.error()
    assert all((m.to_numpy() == np.uint64(SENTINEL)).all() for m in call.match) and call.record() == rep
    call = Call(kind)                                                           # neither
    call.n_table = call.n = 0
    assert call() == 0, call.error()
    assert call.record() == {k: 0 for k in REPORT_FIELDS}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_checked_mode_names_side_column_and_row(kind, fname):
    pl, pair = backends.planner(kind), FIELDS[fname]
    table, base, table_key, keys, match, rep = case(fname, 120, 300, 2, 2, 40, "nonzero", ("zero", None))
    p_words = [(pair.bf.p >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(pair.bf.nlimbs)]          # p itself: the smallest non-canonical value
    V = len(p_words)
    try:
        pl.checked(True)
        # a key column and the mask column of the table; a key column and a mask column of the probe side
        for side, col, row in (("d_table", 1, 17), ("d_table", 2, 119), ("d_base", 3, 299), ("d_base", 5, 0)):
            call = Call(kind, fname)
            w = pair.base_words((table if side == "d_table" else base)[col])
            w[V * row:V * (row + 1)] = p_words
            keep = GpuVec.from_numpy(pl, w, pair.base_field)
            (call.table_ptrs if side == "d_table" else call.base_ptrs)[col] = keep.ptr
            assert call() == INVALID, call.error()
            msg = call.error()
            assert "canonical" in msg and "ms_join_rows" in msg and side in msg and f"column {col}, row {row};" in msg, msg
            assert ("d_base" if side == "d_table" else "d_table") not in msg, msg
            call.unchanged()
        # a column that no key names is not read, so it is not scanned: the payload column and a spare mask column hold all ones
        tw, bw = [pair.base_words(c) for c in table], [pair.base_words(c) for c in base]
        tw[4][:] = 0xFFFFFFFFFFFFFFFF
        tw[3][:] = 0xFFFFFFFFFFFFFFFF
        bw[4][:] = 0xFFFFFFFFFFFFFFFF
        d_table, d_base = (Matrix([GpuVec.from_numpy(pl, w, pair.base_field) for w in ws]) for ws in (tw, bw))
        matches, report = join_rows(pl, d_table, table_key, d_base, keys)
        check(matches, report, match, rep, fname)
    finally:
        pl.checked(False)


def test_python_mirror_argument_checks():
    pl, pair = backends.planner("emu"), FIELDS["fp"]
    d_table, d_base = upload(pl, pair, [[1, 2], [5, 6]]), upload(pl, pair, [[2, 1, 3], [0, 0, 0]])
    with pytest.raises(MsError) as err:
        join_rows(pl, d_table, LookupTuple([0]), d_base, [LookupTuple([9])])
    assert err.value.code == INVALID and "out of range" in str(err.value) and "d_base" in str(err.value)
    with pytest.raises(MsError) as err:
        join_rows(pl, d_table, LookupTuple([2]), d_base, [LookupTuple([0])])
    assert err.value.code == INVALID and "out of range" in str(err.value) and "d_table" in str(err.value)
    with pytest.raises(ValueError):
        join_rows(pl, d_table, LookupTuple([0]), d_base, [LookupTuple([0, 1])])                # widths differ
    with pytest.raises(ValueError):
        join_rows(pl, d_table, LookupTuple([0]), d_base, [LookupTuple([0])] * 9)
    with pytest.raises(ValueError):
        join_rows(pl, d_table, LookupTuple([0]), upload(pl, FIELDS["fp252"], [[1]]), [LookupTuple([0])])      # fields differ
    with pytest.raises(ValueError):
        join_rows(pl, [d_table.columns[0], d_base.columns[0]], LookupTuple([0]), d_base, [LookupTuple([0])])      # lengths differ
    assert (extension.JOIN_MAX_WIDTH, extension.JOIN_MAX_SETS, extension.JOIN_NONE) == (4, 8, NONE)
    matches, report = join_rows(pl, d_table, LookupTuple([0]), d_base, [LookupTuple([0])])
    assert isinstance(matches[0], DeviceIndex) and list(matches[0].to_numpy()) == [1, 0, NONE]
    assert not report and report.missing == 1 and report.first_missing_values() == [3]
    matches, report = join_rows(pl, d_table, LookupTuple([0]), d_base, [])
    assert matches == [] and report.check() is report and report.first_missing_values() is None and report.table_active == 2
    fetched, report = fetch_columns(pl, d_table, LookupTuple([0]), d_base, LookupTuple([0]), [1])
    assert list(fetched.columns[0].to_numpy()) == list(pair.base_words([6, 5, 0]))
