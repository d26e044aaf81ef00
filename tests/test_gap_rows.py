"""ms_gap_plan and ms_gap_fill (include/ministark_hip_gaps.h) against the loops on Python integers (tests/gaps_ref.py): every word of start,
of the report and of the filled columns.

    T = 1024   positions a workgroup of the plan handles (msgap::TILE: 256 threads, 4 positions each; waves of 64)
    R = 256    tiles past which the scan of the tile sums takes one more round (msgap::SCAN_ROUND)
    U = 1024   output rows a workgroup of the fill owns (msgap::OUT_TILE)
    S = 2048   entries of start[] a fill workgroup stages in LDS (msgap::SLICE); a longer slice is searched in global memory

Lengths 1, 2, 3, T-1, T, T+1, 2T+1 on both backends and R T + 3 on the device only, both fields, the three masks in rotation, 0..3 group
columns, with and without a permutation (entries >= n_src included); neighbour pairs across a wave and a tile edge; gaps across an output
tile edge and one longer than 3 U; runs of inactive positions around S; no and one position active, rows_out = 0; n_out below, at and above
rows_out; gaps at the cap of 2^32; a difference in a high limb only; unordered counters; a counter that wraps past p in the padding; every
column kind and 128 columns; the plain select; plain padding in the five shapes of pad_*_rows; five equal runs; refusals, overlaps,
unsupported cases, checked mode and the Python mirror's own checks."""
import ctypes
import functools

import numpy as np
import pytest

from tests import backends
from tests import gaps_ref
from tests.ext_ref import PAIRS
from ministark_amd import DeviceIndex, GapError, GapSpec, GpuVec, Matrix, extension, gap_fill, gap_plan
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, STARK252_FP as F252F
from ministark_amd._lib import GapColumnRecord, GapReportRecord, GapSpecRecord, MsError

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = {"fp": PAIRS["fp_fp"], "fp252": PAIRS["fp252_fp252"]}
T, R, U, S = 1024, 256, 1024, 2048
LENGTHS = [1, 2, 3, T - 1, T, T + 1, 2 * T + 1]
INVALID, UNSUPPORTED = -1, -2
SENTINEL = 0xA5A5A5A5A5A5A5A5
MASKS = [None, "nonzero", "zero"]
REPORT = ["active", "rows_out", "gaps", "max_gap", "unordered", "first_unordered", "saturated"]
MEMORY = [("counter", 0), ("copy", 1), ("zero", 2), ("flag", None)]


def upload(pl, pair, base):
    return Matrix([GpuVec.from_numpy(pl, pair.base_words(c), pair.base_field) for c in base])


def report_dict(report):
    d = {k: getattr(report, k) for k in REPORT}
    if d["first_unordered"] is None:
        d["first_unordered"] = gaps_ref.NONE_UNORDERED
    return d


def run(kind, fname, base, spec, columns, perm=None, n=None, n_out=None, pad=5, runs=1, rows=None):
    """plan and fill on the backend, compare start, report and columns with the reference; -> (start, report, columns) of the reference.
    n_out: default rows_out + pad.  rows: compare these output rows only (the first n_out are still written); a function of n_out gives them."""
    pl, pair = backends.planner(kind), FIELDS[fname]
    start, rep = gaps_ref.plan(base, spec, perm, n)
    n_out = rep["rows_out"] + pad if n_out is None else n_out
    rows = rows(n_out) if callable(rows) else rows
    want = gaps_ref.fill(base, start, columns, n_out, pair.bf.p, perm, rows)
    want_words = [pair.base_words(c) for c in want]
    d_base = upload(pl, pair, base)
    d_perm = None if perm is None else DeviceIndex.from_numpy(pl, np.array(perm, dtype=np.uint32))
    V = pair.bf.nlimbs
    for _ in range(runs):
        plan = gap_plan(pl, d_base, spec, perm=d_perm, n=n)
        got = plan.start_to_numpy()
        assert [int(v) for v in got] == start, (fname, spec._record())
        assert report_dict(plan.report) == rep, (fname, repr(plan.report), rep)
        out = gap_fill(pl, d_base, plan, columns, n_out=n_out)
        assert out.num_cols() == len(columns) and out.num_rows() == n_out
        for c, col in enumerate(out.columns):
            g = col.to_numpy()
            if rows is not None:
                g = g.reshape(-1, V)[list(rows)].ravel()
            bad = np.nonzero(g != want_words[c])[0]
            assert bad.size == 0, (fname, columns[c], f"{bad.size} words differ, the first at row {int(bad[0]) // V}")
    for c, v in zip(d_base.columns, base):                                      # the inputs are only read
        assert np.array_equal(c.to_numpy(), pair.base_words(v))
    return start, rep, want


@functools.lru_cache(maxsize=None)
def structured(n, ngroup, with_perm, seed=0, steps=(1, 1, 1, 2, 3, 9)):
    """-> (base, perm): base columns 0 = a counter that ascends along the positions by `steps`, 1 and 2 = values, 3.. = the group columns
    (runs of equal values), last = a mask column (0 on about a third of the rows).  with_perm: the rows lie shuffled among n + 3 and
    perm[j] names the row of position j; from n = 3 on, a few entries are no rows at all (>= n_src)."""
    rng = np.random.default_rng([n, ngroup, int(with_perm), seed])
    counter = [int(v) for v in np.cumsum(rng.choice(steps, size=n))]
    cols = [counter, [int(v) for v in rng.integers(0, 1 << 62, size=n)], [int(v) for v in rng.integers(1, 1 << 40, size=n)]]
    for _ in range(ngroup):
        cols.append([int(v) for v in np.cumsum(rng.integers(0, 5, size=n) == 0)])
    cols.append([int(v) if k else 0 for v, k in zip(rng.integers(1, 1 << 62, size=n), rng.integers(0, 3, size=n))])
    if not with_perm:
        return cols, None
    n_src = n + 3
    where = [int(v) for v in rng.permutation(n_src)]
    base = [[7] * n_src for _ in cols]
    for c, col in enumerate(cols):
        for j in range(n):
            base[c][where[j]] = col[j]
    perm = where[:n]
    if n >= 3:
        for j, v in zip(sorted({n // 2, n - 1, 1}), (n_src, 0xFFFFFFFF, n_src + 5)):
            perm[j] = v
    return base, perm


def spec_for(ngroup, mask, counter=0):
    return GapSpec(group=range(3, 3 + ngroup), counter=counter, mask=None if mask is None else (mask, 3 + ngroup))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_fields_masks_groups_and_permutations(kind, fname, n):
    for ngroup in (0, 1, 2, 3):
        with_perm = (ngroup + n) % 2 == 1
        base, perm = structured(n, ngroup, with_perm)
        _, rep, _ = run(kind, fname, base, spec_for(ngroup, MASKS[(ngroup + n) % 3]), MEMORY, perm=None if perm is None else list(perm))
        assert rep["unordered"] == 0 or with_perm


@pytest.mark.gpu
@pytest.mark.parametrize("fname", list(FIELDS))
def test_past_one_round_of_the_scan(fname):
    n = R * T + 3
    base, _ = structured(n, 1, False, steps=(1, 1, 1, 2))
    rows = None if fname == "fp" else (lambda n_out: list(range(300)) + list(range(n_out // 2, n_out // 2 + 300)) + list(range(n_out - 300, n_out)))
    _, rep, _ = run("hip", fname, base, spec_for(1, "nonzero"), MEMORY, rows=rows)
    assert rep["rows_out"] > n // 2 and rep["gaps"] > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_pairs_that_straddle_a_wave_edge_and_a_tile_edge(kind, fname):
    n = 2 * T + 1
    jumps = {63: 6, 255: 2, T - 1: 8, 2 * T - 1: 4}                             # (63, 64): two waves; (T-1, T), (2T-1, 2T): two tiles
    counter, at = [], 10
    for j in range(n):
        counter.append(at)
        at += jumps.get(j, 1)
    base = [counter, list(range(n)), [3] * n, [1] * n]
    start, rep, _ = run(kind, fname, base, GapSpec(group=[3], counter=0), MEMORY)
    assert (rep["gaps"], rep["max_gap"], rep["rows_out"]) == (4, 7, n + 5 + 1 + 7 + 3)
    assert start[T] - start[T - 1] == 8 and start[64] - start[63] == 6
    # the same pairs in different groups: no gap
    _, rep, _ = run(kind, fname, [counter, list(range(n)), [3] * n, [int(j > 63) + int(j > T - 1) + int(j > 2 * T - 1) + int(j > 255) for j in range(n)]],
                    GapSpec(group=[3], counter=0), MEMORY)
    assert rep["gaps"] == 0 and rep["rows_out"] == n


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_gaps_across_an_output_tile_edge_and_one_longer_than_three_tiles(kind, fname):
    counter = [0, 1, U + 12, U + 13, 4 * U + 80, 4 * U + 81, 4 * U + 90]       # rows 1 .. U+11 come from position 1, a gap of 3U+66 after position 3
    base = [counter, [5, 6, 7, 8, 9, 10, 11], [21, 22, 23, 24, 25, 26, 27]]
    start, rep, _ = run(kind, fname, base, GapSpec(counter=0), MEMORY, pad=U + 3)
    assert rep["max_gap"] == 3 * U + 66 and start[1] < U < start[2] - 1 and rep["rows_out"] == 4 * U + 91
    assert any(start[3] < t * U and (t + 1) * U <= start[4] for t in range(5))   # a whole output tile has one source row


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [S - 2, S - 1, S, S + 1])
def test_runs_of_inactive_positions_around_the_slice_capacity(kind, m):
    """m inactive positions between two active ones: the slice of an output tile that holds both has m + 2 entries; it is staged up to S
    entries (m = S - 2) and searched in global memory from m = S - 1 on"""
    head, tail = 5, 4
    n = head + m + tail
    flags = [1] * head + [0] * m + [1] * tail
    counter = [3 * j for j in range(n)]
    base = [counter, list(range(100, 100 + n)), list(range(1, n + 1)), flags]
    for mk, col in (("nonzero", flags), ("zero", [1 - f for f in flags])):
        base[3] = col
        start, rep, _ = run(kind, "fp", base, GapSpec(counter=0, mask=(mk, 3)), MEMORY)
        assert rep["active"] == head + tail and start[head] == start[head + m] and rep["rows_out"] == 3 * (head - 1) + 1 + 3 * (tail - 1) + 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_no_position_and_one_position_active(kind, fname):
    for n in (1, 5, T + 1):
        base = [list(range(2, 2 * n + 2, 2)), list(range(50, 50 + n)), list(range(1, n + 1))]
        for hot in (None, 0, n // 2, n - 1):
            for mk in ("nonzero", "zero"):
                flags = [int((i == hot) == (mk == "nonzero")) for i in range(n)]
                start, rep, want = run(kind, fname, base + [flags], GapSpec(counter=0, mask=(mk, 3)), MEMORY, n_out=4)
                assert rep["active"] == rep["rows_out"] == int(hot is not None)
                if hot is None:                                                 # rows_out = 0 with n_out > 0: zero elements and the flag set
                    assert want == [[0] * 4, [0] * 4, [0] * 4, [1] * 4]
                else:
                    assert want[0] == [base[0][hot] + k for k in range(4)] and want[3] == [0, 1, 1, 1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_truncation_exact_fit_and_padding(kind, fname):
    base, _ = structured(300, 1, False)
    spec = spec_for(1, "nonzero")
    _, rep = gaps_ref.plan(base, spec)
    for n_out in (1, rep["rows_out"] - 3, rep["rows_out"], rep["rows_out"] + 9, 2 * U + 1):
        run(kind, fname, base, spec, MEMORY, n_out=n_out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_gaps_at_the_cap_and_the_widest_difference(kind, fname):
    """d - 1 = 2^32 - 1, 2^32 (the cap, not clipped), 2^32 + 1 (clipped), and 0 -> p - 1; the plan in full, the fill for its first 300 rows"""
    p = FIELDS[fname].bf.p
    for d, gap, sat in ((1 << 32, (1 << 32) - 1, 0), ((1 << 32) + 1, 1 << 32, 0), ((1 << 32) + 2, 1 << 32, 1), (p - 1, 1 << 32, 1)):
        lo = 0 if d == p - 1 else 77
        base = [[lo, lo + d, lo + d + 1] if d != p - 1 else [lo, lo + d, 5], [1, 2, 3], [4, 5, 6]]
        start, rep, _ = run(kind, fname, base, GapSpec(counter=0), MEMORY, n_out=300)
        assert start[1] == 1 + gap and rep["saturated"] == sat and rep["max_gap"] == gap
        assert rep["unordered"] == int(d == p - 1)                               # p - 1 -> 5 descends
    pl = backends.planner(kind)
    plan = gap_plan(pl, upload(pl, FIELDS[fname], [[0, (1 << 32) + 2]]), GapSpec(counter=0))
    with pytest.raises(GapError, match="clipped"):
        plan.report.check()


@pytest.mark.parametrize("kind", KINDS)
def test_a_difference_in_a_high_limb_only(kind):
    for limb in (1, 2, 3):
        for low in (0, 1, 5):
            a = 9 + (3 << 64)
            base = [[a, a + (1 << (64 * limb)) + low - (5 if low == 5 else 0), 0], [1, 2, 3], [4, 5, 6]]
            base[0][2] = base[0][1] + 1
            start, rep, _ = run(kind, "fp252", base, GapSpec(counter=0), MEMORY, n_out=300)
            assert start[1] == 1 + (1 << 32) and rep["saturated"] == 1 and rep["unordered"] == 0
    # the low limb descends while a high limb ascends, and the other way round
    base = [[(1 << 64) + 9, (2 << 64) + 3, (2 << 64) + 4, (1 << 64) + 900], [1, 2, 3, 4], [4, 5, 6, 7]]
    _, rep, _ = run(kind, "fp252", base, GapSpec(counter=0), MEMORY, n_out=300)
    assert (rep["saturated"], rep["unordered"], rep["first_unordered"]) == (1, 1, 2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_counters_that_do_not_ascend_are_counted_and_named(kind, fname):
    n = T + 3
    counter = list(range(10, 10 + n))
    counter[700] = counter[699]                                                 # d = 0 at 699
    counter[T] = 3                                                              # d < 0 at T - 1; 3 -> 10 + T + 1 is a gap
    base = [counter, list(range(n)), [2] * n]
    _, rep, _ = run(kind, fname, base, GapSpec(counter=0), MEMORY)
    assert (rep["unordered"], rep["first_unordered"]) == (2, 699)
    pl = backends.planner(kind)
    plan = gap_plan(pl, upload(pl, FIELDS[fname], base), GapSpec(counter=0))
    with pytest.raises(GapError, match="699"):
        plan.report.check()
    assert "unordered=2" in repr(plan.report)
    good = gap_plan(pl, upload(pl, FIELDS[fname], [[1, 2, 5]]), GapSpec(counter=0))
    assert good.report.check() is good.report and good.report.first_unordered is None


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_the_counter_wraps_past_p_in_the_padding(kind, fname):
    p = FIELDS[fname].bf.p
    base = [[p - 9, p - 6, p - 2], [1, 2, 3], [4, 5, 6]]
    _, rep, want = run(kind, fname, base, GapSpec(counter=0), MEMORY, pad=6)
    assert rep["rows_out"] == 8 and want[0][-7:] == [p - 2, p - 1, 0, 1, 2, 3, 4] and want[3][-7:] == [0] + [1] * 6


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_each_column_kind_and_128_columns(kind, fname):
    base, _ = structured(300, 1, False)
    kinds = ["copy", "zero", "counter", "flag"]
    for ncols in (1, 2, 128):
        columns = [(kinds[(c + ncols) % 4], None if kinds[(c + ncols) % 4] == "flag" else c % 3) for c in range(ncols)]
        run(kind, fname, base, spec_for(1, "zero"), columns)
    for k in kinds:
        run(kind, fname, base, spec_for(1, None), [(k, None if k == "flag" else 2)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_without_a_counter_it_is_a_stable_select(kind, fname):
    for n in (7, T + 1):
        base, _ = structured(n, 2, False)
        for mk in ("nonzero", "zero"):
            spec = GapSpec(group=[3, 4], counter=None, mask=(mk, 5))
            keep = [i for i in range(n) if (base[5][i] != 0) == (mk == "nonzero")]
            start, rep, want = run(kind, fname, base, spec, [("copy", 0), ("copy", 1), ("copy", 5)], pad=0)
            assert rep["rows_out"] == len(keep) and rep["gaps"] == 0
            assert want == [[base[c][i] for i in keep] for c in (0, 1, 5)]


PAD_SHAPES = {"processor": [("counter", 0), ("copy", 1), ("zero", 2), ("zero", 3), ("copy", 4), ("copy", 5), ("copy", 6), ("flag", None)],
              "memory": [("counter", 0), ("copy", 1), ("copy", 2), ("flag", None)],
              "instruction": [("copy", 0), ("zero", 1), ("zero", 2)],
              "input": [("zero", 0)],
              "output": [("zero", 0)]}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", list(PAD_SHAPES))
def test_plain_padding_in_the_shapes_of_the_reference_tables(kind, shape):
    """pad_processor_rows, pad_memory_rows, pad_instruction_rows, pad_input_rows, pad_output_rows (examples/brainfuck/vm.rs:282-336): no mask,
    no counter; the table's rows come out as they are and the padding rows as those loops build them"""
    columns = PAD_SHAPES[shape]
    n, n_out = 37, 64
    rng = np.random.default_rng(len(columns))
    base = [[int(v) for v in rng.integers(1, 1 << 50, size=n)] for _ in range(7)]
    base[0] = list(range(n))
    _, rep, want = run(kind, "fp", base, GapSpec(), columns, n_out=n_out)
    assert rep["rows_out"] == n
    rows = [[base[src][i] if kind_ != "flag" else 0 for kind_, src in columns] for i in range(n)]
    while len(rows) < n_out:                                                    # the reference's loops, column kind by column kind
        last = rows[-1]
        rows.append([last[c] + 1 if k == "counter" else last[c] if k == "copy" else 0 if k == "zero" else 1 for c, (k, _) in enumerate(columns)])
    assert want == [[r[c] for r in rows] for c in range(len(columns))]


@pytest.mark.gpu
@pytest.mark.parametrize("fname", list(FIELDS))
def test_five_runs_give_one_result(fname):
    base, perm = structured(2 * T + 1, 2, True)
    run("hip", fname, base, spec_for(2, "nonzero"), MEMORY, perm=list(perm), runs=5)


# ---- refusals and empty cases ----------------------------------------------------------------------------------------------------------
class PlanCall:
    """one raw ms_gap_plan whose arguments a test can bend; d_start and d_report are filled with a sentinel"""

    def __init__(self, kind, fname="fp", n=300):
        self.pl, self.pair = backends.planner(kind), FIELDS[fname]
        self.base, perm = structured(n, 2, True)                               # columns 0 counter, 1, 2 values, 3, 4 group, 5 mask; n + 3 rows
        self.perm_host = list(perm)
        self.d_base = upload(self.pl, self.pair, self.base)
        self.field, self.n, self.n_src, self.V = self.pair.base_field, n, n + 3, self.pair.bf.nlimbs
        self.base_ptrs = [c.ptr for c in self.d_base.columns]
        self.spec = GapSpec(group=[3, 4], counter=0, mask=("nonzero", 5))._record()
        self.perm = DeviceIndex.from_numpy(self.pl, np.array(perm, dtype=np.uint32))
        self.start = GpuVec.from_numpy(self.pl, np.full(n + 1, SENTINEL, dtype=np.uint64), FP)
        self.report = GpuVec.from_numpy(self.pl, np.full(8, SENTINEL, dtype=np.uint64), FP)
        self.perm_ptr, self.start_ptr, self.report_ptr, self.null, self.handle = self.perm.ptr, self.start.ptr, self.report.ptr, (), self.pl.handle

    def __call__(self):
        rec = np.array(self.spec, dtype=np.int32)
        VP = ctypes.c_void_p
        return self.pl.lib.ms_gap_plan(self.handle, self.field, self.n_src, None if "base" in self.null else (VP * max(1, len(self.base_ptrs)))(*self.base_ptrs),
                                       len(self.base_ptrs), None if "spec" in self.null else rec.ctypes.data, self.perm_ptr, self.n, self.start_ptr, self.report_ptr)

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self):
        assert (self.start.to_numpy() == np.uint64(SENTINEL)).all() and (self.report.to_numpy() == np.uint64(SENTINEL)).all()


def want_report(rep):
    return [rep[k] for k in REPORT] + [0]


@pytest.mark.parametrize("kind", KINDS)
def test_the_bent_plan_call_is_accepted_unbent(kind):
    call = PlanCall(kind)
    assert call() == 0, call.error()
    start, rep = gaps_ref.plan(call.base, GapSpec(group=[3, 4], counter=0, mask=("nonzero", 5)), call.perm_host)
    assert [int(v) for v in call.start.to_numpy()] == start and [int(v) for v in call.report.to_numpy()] == want_report(rep)
    call = PlanCall(kind)                                                       # no permutation: the identity over the first n rows
    call.perm_ptr = None
    assert call() == 0, call.error()
    start, rep = gaps_ref.plan(call.base, GapSpec(group=[3, 4], counter=0, mask=("nonzero", 5)), None, n=call.n)
    assert [int(v) for v in call.start.to_numpy()] == start and [int(v) for v in call.report.to_numpy()] == want_report(rep)


@pytest.mark.parametrize("kind", KINDS)
def test_plan_null_arguments_indices_and_kinds_are_refused(kind):
    nbase = 6
    bends = [lambda c: setattr(c, "handle", None), lambda c: setattr(c, "null", ("base",)), lambda c: setattr(c, "null", ("spec",)),
             lambda c: setattr(c, "start_ptr", None), lambda c: setattr(c, "report_ptr", None),
             lambda c: c.base_ptrs.__setitem__(2, None), lambda c: setattr(c, "field", 7),
             lambda c: c.spec.__setitem__(3, 4), lambda c: c.spec.__setitem__(3, -1),                                  # ngroup
             lambda c: c.spec.__setitem__(1, nbase), lambda c: c.spec.__setitem__(0, -1),                              # a group column
             lambda c: c.spec.__setitem__(4, nbase),                                                                   # the counter
             lambda c: c.spec.__setitem__(6, nbase), lambda c: c.spec.__setitem__(6, -1),                              # the mask column
             lambda c: c.spec.__setitem__(5, 3), lambda c: c.spec.__setitem__(5, -1)]                                  # the mask kind
    for k, bend in enumerate(bends):
        call = PlanCall(kind)
        assert len(call.base_ptrs) == nbase
        bend(call)
        assert call() == INVALID, (k, call.error())
        call.unchanged()
    call = PlanCall(kind)                                                       # what is not read is not checked: group columns past ngroup, an unmasked spec's mask column
    call.spec[2] = 99
    assert call() == 0, call.error()
    call = PlanCall(kind)
    call.spec[5], call.spec[6] = 0, 99
    assert call() == 0, call.error()
    call = PlanCall(kind)                                                       # any negative counter: no gaps
    call.spec[4] = -7
    assert call() == 0, call.error()
    assert int(call.report.to_numpy()[2]) == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_plan_outputs_that_overlap_are_refused(kind, fname):
    def refused(bend):
        call = PlanCall(kind, fname)
        bend(call)
        assert call() == INVALID and "overlap" in call.error(), call.error()
        call.unchanged()
    col = lambda c: 8 * c.V * c.n_src
    refused(lambda c: setattr(c, "start_ptr", c.base_ptrs[0]))                  # the counter
    refused(lambda c: setattr(c, "start_ptr", c.base_ptrs[4]))                  # a group column
    refused(lambda c: setattr(c, "start_ptr", c.base_ptrs[5] + col(c) - 8))     # the last bytes of the mask column
    refused(lambda c: setattr(c, "report_ptr", c.base_ptrs[3] + 8))
    refused(lambda c: setattr(c, "start_ptr", c.perm_ptr))                      # the permutation
    refused(lambda c: setattr(c, "report_ptr", c.perm_ptr + 4 * c.n - 4))
    refused(lambda c: setattr(c, "report_ptr", c.start_ptr))                    # each other
    refused(lambda c: setattr(c, "report_ptr", c.start_ptr + 8 * c.n))
    call = PlanCall(kind, fname)                                                # column 1 is not named by the spec: it may take the report
    call.report_ptr = call.base_ptrs[1]
    assert call() == 0, call.error()


@pytest.mark.parametrize("kind", KINDS)
def test_plan_unsupported_cases_and_no_positions(kind):
    for bend in (lambda c: setattr(c, "field", FQ3F), lambda c: setattr(c, "n", (1 << 30) + 1), lambda c: setattr(c, "n_src", (1 << 32) + 1)):
        call = PlanCall(kind)
        bend(call)
        assert call() == UNSUPPORTED, call.error()
        call.unchanged()
    call = PlanCall(kind)
    call.n = 0
    assert call() == 0, call.error()
    got = call.start.to_numpy()
    assert int(got[0]) == 0 and (got[1:] == np.uint64(SENTINEL)).all()
    assert [int(v) for v in call.report.to_numpy()] == [0, 0, 0, 0, 0, (1 << 64) - 1, 0, 0]
    pl = backends.planner(kind)
    d_base = upload(pl, FIELDS["fp"], [[3, 1, 2]])
    plan = gap_plan(pl, d_base, GapSpec(counter=0), n=0)
    assert (plan.report.rows_out, plan.report.first_unordered, plan.n) == (0, None, 0)
    out = gap_fill(pl, d_base, plan, [("copy", 0), ("flag", None)], n_out=3)     # no positions: the table is empty
    assert [int(v) for v in out.columns[0].to_numpy()] == [0, 0, 0] and np.array_equal(out.columns[1].to_numpy(), FIELDS["fp"].base_words([1, 1, 1]))
    assert gap_fill(pl, d_base, plan, [("copy", 0)]).num_rows() == 1             # the least power of two >= max(rows_out, 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_plan_checked_mode_names_column_and_row(kind, fname):
    pl, pair = backends.planner(kind), FIELDS[fname]
    p_words = [(pair.bf.p >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(pair.bf.nlimbs)]         # p itself: the smallest non-canonical value
    V = len(p_words)
    try:
        pl.checked(True)
        for col, row in ((0, 17), (4, 302), (5, 0)):                            # the counter, a group column, the mask column
            call = PlanCall(kind, fname)
            w = pair.base_words(call.base[col])
            w[V * row:V * (row + 1)] = p_words
            keep = GpuVec.from_numpy(pl, w, pair.base_field)
            call.base_ptrs[col] = keep.ptr
            assert call() == INVALID, call.error()
            msg = call.error()
            assert "canonical" in msg and "ms_gap_plan" in msg and "d_base" in msg and f"column {col}, row {row};" in msg, msg
            call.unchanged()
        call = PlanCall(kind, fname)                                            # a column that the spec does not name is not scanned
        keep = GpuVec.from_numpy(pl, np.full(V * call.n_src, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), pair.base_field)
        call.base_ptrs[2] = keep.ptr
        assert call() == 0, call.error()
    finally:
        pl.checked(False)


class FillCall:
    """one raw ms_gap_fill over a plan that was made unbent; the destinations are filled with a sentinel"""

    def __init__(self, kind, fname="fp", n=300, n_out=700):
        self.plan = PlanCall(kind, fname, n)
        assert self.plan() == 0, self.plan.error()
        p = self.plan
        self.pl, self.pair, self.field, self.n, self.n_src, self.V, self.n_out = p.pl, p.pair, p.field, n, p.n_src, p.V, n_out
        self.base_ptrs, self.perm_ptr, self.start_ptr, self.handle = list(p.base_ptrs), p.perm_ptr, p.start_ptr, p.handle
        self.columns = [2, 0, 0, 1, 1, 2, 3, 0]                                  # counter 0, copy 1, zero 2, flag
        self.dst = [GpuVec.from_numpy(self.pl, np.full(self.V * n_out, SENTINEL, dtype=np.uint64), self.field) for _ in range(4)]
        self.dst_ptrs, self.ncols, self.null = [d.ptr for d in self.dst], 4, ()

    def __call__(self):
        rec = np.array(self.columns, dtype=np.int32)
        VP = ctypes.c_void_p
        return self.pl.lib.ms_gap_fill(self.handle, self.field, self.n_src, None if "base" in self.null else (VP * len(self.base_ptrs))(*self.base_ptrs),
                                       len(self.base_ptrs), self.perm_ptr, self.n, self.start_ptr, None if "columns" in self.null else rec.ctypes.data,
                                       None if "dst" in self.null else (VP * len(self.dst_ptrs))(*self.dst_ptrs), self.ncols, self.n_out)

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self):
        assert all((d.to_numpy() == np.uint64(SENTINEL)).all() for d in self.dst)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fname", list(FIELDS))
def test_fill_refusals(kind, fname):
    call = FillCall(kind, fname)
    assert call() == 0, call.error()
    spec = GapSpec(group=[3, 4], counter=0, mask=("nonzero", 5))
    start, _ = gaps_ref.plan(call.plan.base, spec, call.plan.perm_host)
    want = gaps_ref.fill(call.plan.base, start, MEMORY, call.n_out, call.pair.bf.p, call.plan.perm_host)
    for d, w in zip(call.dst, want):
        assert np.array_equal(d.to_numpy(), call.pair.base_words(w))
    bends = [lambda c: setattr(c, "handle", None), lambda c: setattr(c, "null", ("base",)), lambda c: setattr(c, "null", ("columns",)),
             lambda c: setattr(c, "null", ("dst",)), lambda c: setattr(c, "start_ptr", None),
             lambda c: c.base_ptrs.__setitem__(4, None), lambda c: c.dst_ptrs.__setitem__(2, None),
             lambda c: setattr(c, "field", 7), lambda c: setattr(c, "ncols", 0), lambda c: setattr(c, "ncols", 129),
             lambda c: c.columns.__setitem__(0, 4), lambda c: c.columns.__setitem__(2, -1),                            # a kind
             lambda c: c.columns.__setitem__(1, 6), lambda c: c.columns.__setitem__(3, -1)]                            # a source column
    for k, bend in enumerate(bends):
        call = FillCall(kind, fname)
        if k == 9:
            call.columns, call.dst_ptrs = call.columns * 33, call.dst_ptrs * 33
        bend(call)
        assert call() == INVALID, (k, call.error())
        call.unchanged()
    call = FillCall(kind, fname)                                                # a flag's source is not read
    call.columns[7] = 99
    assert call() == 0, call.error()
    elem = 8 * call.V
    overlaps = [lambda c: c.dst_ptrs.__setitem__(0, c.base_ptrs[0]),                                  # a source
                lambda c: c.dst_ptrs.__setitem__(1, c.base_ptrs[2] + elem * (c.n_src - 1)),           # the last element of another
                lambda c: c.dst_ptrs.__setitem__(2, c.perm_ptr),                                      # the permutation
                lambda c: c.dst_ptrs.__setitem__(3, c.start_ptr + 8 * c.n),                           # start[n]
                lambda c: c.dst_ptrs.__setitem__(2, c.dst_ptrs[0]),                                   # another destination
                lambda c: c.dst_ptrs.__setitem__(1, c.dst_ptrs[3] + elem * (c.n_out - 1))]
    for k, bend in enumerate(overlaps):
        call = FillCall(kind, fname)
        bend(call)
        assert call() == INVALID and "overlap" in call.error(), (k, call.error())
        call.unchanged()
    for bend in (lambda c: setattr(c, "field", FQ3F), lambda c: setattr(c, "n", (1 << 30) + 1), lambda c: setattr(c, "n_out", (1 << 30) + 1),
                 lambda c: setattr(c, "n_src", (1 << 32) + 1)):
        call = FillCall(kind, fname)
        bend(call)
        assert call() == UNSUPPORTED, call.error()
        call.unchanged()
    call = FillCall(kind, fname)                                                # no output rows: accepted, nothing written
    call.n_out = 0
    assert call() == 0, call.error()
    call.unchanged()


@pytest.mark.parametrize("kind", KINDS)
def test_fill_stays_in_bounds_whatever_start_holds(kind):
    """start[] that no plan wrote: descending, huge, zero.  The rows are not defined; the call is accepted, and under the simulator a read or
    write out of bounds would be one of malloc'd memory"""
    rng = np.random.default_rng(3)
    for junk in (np.arange(301, 0, -1), rng.integers(0, 1 << 63, size=301), np.zeros(301), np.full(301, (1 << 64) - 1, dtype=np.uint64)):
        call = FillCall(kind)
        keep = GpuVec.from_numpy(call.pl, np.asarray(junk).astype(np.uint64), FP)
        call.start_ptr = keep.ptr
        assert call() == 0, call.error()
        call.pl.sync() if hasattr(call.pl, "sync") else call.dst[0].to_numpy()


@pytest.mark.parametrize("kind", KINDS)
def test_fill_checked_mode_names_column_and_row(kind):
    pl, pair = backends.planner(kind), FIELDS["fp"]
    try:
        pl.checked(True)
        call = FillCall(kind)
        w = pair.base_words(call.plan.base[1])
        w[41] = pair.bf.p
        keep = GpuVec.from_numpy(pl, w, pair.base_field)
        call.base_ptrs[1] = keep.ptr
        assert call() == INVALID, call.error()
        msg = call.error()
        assert "canonical" in msg and "ms_gap_fill" in msg and "column 1, row 41;" in msg, msg
        call.unchanged()
        call = FillCall(kind)                                                   # a column no record names is not scanned
        keep = GpuVec.from_numpy(pl, np.full(call.n_src, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), pair.base_field)
        call.base_ptrs[4] = keep.ptr
        assert call() == 0, call.error()
    finally:
        pl.checked(False)


def test_python_mirror_argument_checks():
    pl, pair = backends.planner("emu"), FIELDS["fp"]
    d_base = upload(pl, pair, [[1, 2, 5], [7, 8, 9]])
    with pytest.raises(MsError) as err:
        gap_plan(pl, d_base, GapSpec(counter=9))
    assert err.value.code == INVALID and "out of range" in str(err.value)
    for bad in (lambda: GapSpec(group=[0, 1, 2, 3]), lambda: GapSpec(counter=-1), lambda: GapSpec(mask=("odd", 1)), lambda: gap_plan(pl, d_base, GapSpec(), n=4),
                lambda: gap_plan(pl, [], GapSpec())):
        with pytest.raises(ValueError):
            bad()
    plan = gap_plan(pl, d_base, GapSpec(counter=0))
    assert [int(v) for v in plan.start_to_numpy()] == [0, 1, 4, 5] and plan.report.rows_out == 5
    for bad in (lambda: gap_fill(pl, d_base, plan, []), lambda: gap_fill(pl, d_base, plan, [("copy", None)]), lambda: gap_fill(pl, d_base, plan, [("twice", 0)]),
                lambda: gap_fill(pl, d_base, plan, [("copy", 0)], n_out=-1), lambda: gap_fill(pl, d_base, plan, [("copy", 0)], out=[GpuVec(pl, 2, FP)], n_out=3),
                lambda: gap_fill(pl, d_base.columns[:1] + [GpuVec(pl, 4, FP)], plan, [("copy", 0)]),
                lambda: gap_fill(pl, [GpuVec(pl, 4, FP)], plan, [("copy", 0)])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(MsError) as err:
        gap_fill(pl, d_base, plan, [("copy", 0), ("copy", 1)], n_out=3, out=d_base)
    assert err.value.code == INVALID and "overlap" in str(err.value)
    out = gap_fill(pl, d_base, plan, [("counter", 0), ("flag", None)])           # n_out: the least power of two >= rows_out
    assert out.num_rows() == 8 and np.array_equal(out.columns[0].to_numpy(), pair.base_words([1, 2, 3, 4, 5, 6, 7, 8]))
    assert np.array_equal(out.columns[1].to_numpy(), pair.base_words([0, 0, 1, 1, 0, 1, 1, 1]))
    keep = [GpuVec.from_numpy(pl, np.full(9, SENTINEL, dtype=np.uint64), FP)]
    got = gap_fill(pl, d_base, plan, [("copy", 1)], n_out=5, out=keep)           # longer destinations: their first n_out elements are filled
    assert got.columns[0] is keep[0] and [int(v) for v in keep[0].to_numpy()[5:]] == [SENTINEL] * 4
    assert (extension.GAP_MAX_GROUP, extension.GAP_MAX_COLUMNS) == (3, 128)
    assert (ctypes.sizeof(GapSpecRecord), ctypes.sizeof(GapReportRecord), ctypes.sizeof(GapColumnRecord)) == (32, 64, 8)
    assert F252F in (f.base_field for f in FIELDS.values())
