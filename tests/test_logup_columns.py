"""ms_build_logup_columns (include/ministark_hip_logup.h) against the sequential loop on Python integers (tests/logup_ref.py), word for word:
lengths around the rows of a workgroup, 0 / 1 / 4 fractions, 0 (the literal 1) / 1 / 8 terms in a numerator, 1 / 8 in a denominator, both
signs, literal-1 and challenge coefficients, offsets that wrap, the three inits, the three masks, inclusive and exclusive output, 1 / 32
columns in a call, the three field pairs -- zero denominators at arbitrary places of a lane's batch, on every row, and on all PER rows of a
lane -- and the refusals, after which the sentinel-filled outputs are unchanged.  The walk of the block sums is one workgroup per column
whose lane t walks ceil(nblocks / 256) blocks: test_block_walk_past_256_blocks runs both sides of that edge."""
import ctypes
import functools

import numpy as np
import pytest

from tests import backends
from tests.logup_ref import PAIRS, reference
from tests.test_extension_columns import walk_words
from ministark_amd import GpuVec, LogUpColumn, Matrix, build_extension_columns, build_logup_columns, extension
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, STARK252_FP as F252F
from ministark_amd._lib import MsError

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
B = extension.ROWS_PER_WORKGROUP           # the rows per workgroup: mslogup::ROWS is msext::ROWS (tests/test_logup_abi.py checks it against the kernels)
PER = 4                                   # rows per lane (tests/test_logup_abi.py)
LENGTHS = [1, 2, 3, 255, 256, 1023, 1024, 1025, 2 * B + 1]
# base columns 0..5 random, 6 a random 0 / non-zero mix, 7 all zero, 8 zero but for the last row, 9 zero on all PER rows of every third lane
NBASE, NCHAL = 10, 5
INVALID, UNSUPPORTED = -1, -2
SENTINEL = 0xA5A5A5A5A5A5A5A5


def offsets(n):
    return [0, 1, -1, n - 1, -n - 1, 5 * n + 2]


def designed_columns(n):
    """ten columns that between them take every path the header describes"""
    o = offsets(n)
    eight = lambda s: [((+1, -1)[(k + s) % 2], (None, 0, 1, 2, 3, 4)[(k + s) % 6], (None, 0, 1, 2, 3, 4, 5)[(3 * k + s) % 7], o[(k + s) % 6]) for k in range(8)]
    den = lambda c0, c1: [(+1, 0, None), (-1, None, c0), (-1, 1, c1)]
    return [
        LogUpColumn(0, [([], [(+1, None, 6)])]),                                                               # 1 / x, x zero at arbitrary places of a lane's batch
        LogUpColumn(("challenge", 1), [([], eight(0)), ([(-1, 2, 3, 1)], [(+1, 0, None), (-1, None, 1, -1)]),
                                       (eight(1), [(-1, None, 2, n - 1)]), (eight(2), eight(3))], inclusive=True),   # 4 fractions: nn = 0, 1, 8, 8; nd = 8, 2, 1, 8
        LogUpColumn(1, []),                                                                                     # no fraction at all: the init everywhere
        LogUpColumn(0, [([(+1, 1, 0)], [(+1, None, 7, 1)]), ([(+1, None, 4)], den(2, 3))], mask=("nonzero", 6)),   # a denominator that is zero on every row, beside a live one
        LogUpColumn(1, [([(+1, None, 5, -n - 1)], [(-1, None, 9)])], inclusive=True),                           # lanes whose PER denominators are all zero
        LogUpColumn(("challenge", 4), [([], [(+1, 2, 3, -1)])], mask=("nonzero", 7)),                           # inactive everywhere
        LogUpColumn(1, [([(+1, 0, 4, n - 1)], [(+1, 1, 5, -n - 1)])], mask=("nonzero", 8), inclusive=True),     # active on the last row only
        LogUpColumn(0, [([(+1, None, 4)], den(2, 3)), ([(-1, None, None)], den(0, 1))], mask=("zero", 7)),      # the lookup rule under a mask that is active everywhere
        LogUpColumn(0, [([(+1, None, None), (+1, 3, None)], [(+1, 2, None)]), ([], [(+1, None, None), (+1, None, None)])], mask=("zero", 6)),   # constants only: (1 + c3) / c2 + 1 / 2
        LogUpColumn(("challenge", 0), [([], [(+1, 1, 6, 5 * n + 2), (-1, 1, 6, 5 * n + 2)])]),                  # x - x: a zero that sum_terms computes
    ]


def random_columns(rng, n, count):
    o = offsets(n)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    term = lambda: (pick((+1, -1)), pick((None,) + tuple(range(NCHAL))), pick((None,) + tuple(range(NBASE))), pick(o))
    fraction = lambda: ([term() for _ in range(pick((0, 1, 3, 8)))], [term() for _ in range(pick((1, 2, 8)))])
    return [LogUpColumn(pick((0, 1, ("challenge", pick(range(NCHAL))))), [fraction() for _ in range(pick((0, 1, 2, 4)))],
                        mask=pick((None, ("nonzero", 6), ("zero", 6), ("nonzero", 8))), inclusive=pick((False, True))) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def case(pair_name, n, count):
    """(base columns, challenges, column records, expected values), computed once and shared by the backends"""
    pair = PAIRS[pair_name]
    rng = np.random.default_rng(2000 * n + count)
    base = [pair.random_base(rng, n) for _ in range(6)]
    base.append([v if k else 0 for v, k in zip(pair.random_base(rng, n), rng.integers(0, 3, size=n))])
    base.append([0] * n)
    base.append([0] * (n - 1) + [7])
    base.append([0 if (i // PER) % 3 == 0 else v or 1 for i, v in enumerate(pair.random_base(rng, n))])
    chal = pair.random_ext(rng, NCHAL)
    columns = designed_columns(n) if count == 10 else random_columns(rng, n, count)
    return base, chal, columns, reference(pair, base, chal, columns)


def upload(pl, pair, base, chal):
    return (Matrix([GpuVec.from_numpy(pl, pair.base_words(c), pair.base_field) for c in base]),
            GpuVec.from_numpy(pl, pair.ext_words(chal), pair.ext_field))


def run_case(kind, pair_name, n, count):
    pl, pair = backends.planner(kind), PAIRS[pair_name]
    base, chal, columns, want = case(pair_name, n, count)
    d_base, d_chal = upload(pl, pair, base, chal)
    got = build_logup_columns(pl, d_base, d_chal, columns, pair.ext_field)
    assert got.num_cols() == count and got.field == pair.ext_field
    for e, (g, w) in enumerate(zip(got.to_numpy(), want)):
        assert np.array_equal(g, pair.ext_words(w)), (pair_name, n, e)
    for c, v in zip(d_base.columns, base):                                    # the inputs are only read
        assert np.array_equal(c.to_numpy(), pair.base_words(v))
    assert np.array_equal(d_chal.to_numpy(), pair.ext_words(chal))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair_name", list(PAIRS))
@pytest.mark.parametrize("n", LENGTHS)
def test_ten_designed_columns(kind, pair_name, n):
    run_case(kind, pair_name, n, 10)


def test_the_designed_inputs_hold_the_zero_denominators_they_are_meant_to():
    base, _, _, want = case("fp_fq3", 1025, 10)
    assert 0 in base[6] and any(base[6]) and any(0 < sum(1 for v in base[6][k:k + PER] if v == 0) < PER for k in range(0, 1024, PER))
    assert not any(base[9][:PER]) and all(base[9][PER:3 * PER]) and not any(base[9][3 * PER:4 * PER])
    assert want[9] == [want[9][0]] * 1025 and want[5] == [want[5][0]] * 1025 and want[2] == [(1, 0, 0)] * 1025
    assert want[6][:-1] == [(1, 0, 0)] * 1024 and want[6][-1] != (1, 0, 0)
    assert want[4][:PER - 1] == [(1, 0, 0)] * (PER - 1) and want[4][PER] != want[4][PER - 1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair_name", list(PAIRS))
@pytest.mark.parametrize("count", [1, 32])
def test_batch_shapes(kind, pair_name, count):
    run_case(kind, pair_name, 1025, count)


# ---- the block walk: 256 blocks (one per lane of logup_blocks) and 257 (two per lane, lane 128 holds the last one) ----------------------
WALK_LENGTHS = [256 * B, 256 * B + 1]
WALK_GUARD = np.array([0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A] * 8, dtype=np.uint64)
WALK_PAIRS = ["fp_fq3", "fp_fp"]          # the reference is a Python loop: the 252-bit pair is left to the sweeps above


def walk_columns():
    """two light columns in one call (gridDim.y = 2: each has its own slice of agg and block_state).  Base columns: 0, 1 values; 2 a 0 /
    non-zero mix that is zero on row 0 and non-zero on the last rows -- the mask of the second column and a denominator with zeros"""
    return [
        LogUpColumn(0, [([], [(+1, 0, None), (-1, None, 0, -1)])], inclusive=True),                            # 1 / (chal0 - col0[i-1])
        LogUpColumn(("challenge", 3), [([(+1, None, 1, +1)], [(+1, None, 2)])], mask=("nonzero", 2)),           # col1[i+1] / col2[i] where col2[i] != 0
    ]


@functools.lru_cache(maxsize=None)
def walk_case(pair_name, n):
    """(columns, base words, challenge words, expected words), computed once and shared by the backends"""
    pair = PAIRS[pair_name]
    rng = np.random.default_rng(91 + n)
    values = lambda: rng.integers(0, pair.bf.p, size=n, dtype=np.uint64).tolist()
    base = [values(), values()]
    keep = rng.integers(0, 3, size=n)
    keep[0], keep[-(B + 3):] = 0, 1
    base.append([(v or 1) if k else 0 for v, k in zip(values(), keep)])
    chal = pair.random_ext(rng, NCHAL)
    columns = walk_columns()
    assert base[2][0] == 0 and all(base[2][-B:]) and 0 in base[2][B:-B - 3]
    want = reference(pair, base, chal, columns)
    assert np.array_equal(walk_words(pair, want[1][-40:], pair.cubic), pair.ext_words(want[1][-40:]))
    return columns, [walk_words(pair, c) for c in base], pair.ext_words(chal), [walk_words(pair, w, pair.cubic) for w in want]


# the simulator takes the longer length (two blocks per lane) only
@pytest.mark.parametrize("kind,n", [pytest.param(kind, n, id=f"{n}-{kind}", marks=[pytest.mark.gpu] if kind == "hip" else [])
                                    for n in WALK_LENGTHS for kind in ("emu", "hip") if kind == "hip" or n == WALK_LENGTHS[1]])
@pytest.mark.parametrize("pair_name", WALK_PAIRS)
def test_block_walk_past_256_blocks(kind, pair_name, n):
    """raw call: every output has guard words behind its last element; the base columns and the challenges are compared after it"""
    pl, pair = backends.planner(kind), PAIRS[pair_name]
    assert -(-n // B) == (256 if n == 256 * B else 257)
    columns, base_w, chal_w, want_w = walk_case(pair_name, n)
    d_base = Matrix([GpuVec.from_numpy(pl, w, pair.base_field) for w in base_w])
    d_chal = GpuVec.from_numpy(pl, chal_w, pair.ext_field)
    call = Call(pl, pair, n, d_base, d_chal, columns)
    V = {FP: 1, FQ3F: 3}[pair.ext_field]
    call.outs = [GpuVec.from_numpy(pl, np.concatenate([np.full(n * V, SENTINEL, dtype=np.uint64), WALK_GUARD]), FP) for _ in columns]
    call.out_ptrs = [o.ptr for o in call.outs]
    assert call() == 0, call.error()
    for e, (o, w) in enumerate(zip(call.outs, want_w)):
        got = o.to_numpy()
        assert np.array_equal(got[n * V:], WALK_GUARD), (pair_name, n, e, "words behind the last element were written")
        bad = np.nonzero(got[:n * V] != w)[0]
        assert bad.size == 0, (pair_name, n, e, f"{bad.size} words differ, the first in row {int(bad[0]) // V}")
    for c, w in zip(d_base.columns, base_w):
        assert np.array_equal(c.to_numpy(), w)
    assert np.array_equal(d_chal.to_numpy(), chal_w)


@pytest.mark.parametrize("kind", KINDS)
def test_zero_rows_and_zero_columns_touch_nothing(kind):
    pl, pair = backends.planner(kind), PAIRS["fp_fq3"]
    base, chal, columns, _ = case("fp_fq3", 3, 10)
    d_base, d_chal = upload(pl, pair, base, chal)
    assert build_logup_columns(pl, d_base, d_chal, [], FQ3F).num_cols() == 0
    call = Call(pl, pair, 3, d_base, d_chal, columns[:2])
    call.n = 0
    assert call() == 0
    call.unchanged()
    call = Call(pl, pair, 3, d_base, d_chal, columns[:2])
    call.next = 0
    assert call() == 0
    call.unchanged()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
class Call:
    """one raw call whose arguments a test can bend; the outputs are filled with a sentinel"""

    def __init__(self, pl, pair, n, d_base, d_chal, columns):
        self.pl, self.pair, self.n, self.columns = pl, pair, n, list(columns)
        self.base_field, self.ext_field = pair.base_field, pair.ext_field
        self.base_ptrs, self.chal_ptr, self.nchal = [c.ptr for c in d_base.columns], d_chal.ptr, len(d_chal)
        V = {FP: 1, FQ3F: 3, F252F: 4}[pair.ext_field]
        self.outs = [GpuVec.from_numpy(pl, np.full(n * V, SENTINEL, dtype=np.uint64), pair.ext_field) for _ in columns]
        self.out_ptrs = [o.ptr for o in self.outs]
        self.keep = (d_base, d_chal)
        self.next = len(self.columns)
        self.bend_records = None          # (recs, fracs, terms) -> None, in place
        self.null = ()                    # of "columns", "fractions", "terms", "base", "outs"

    def __call__(self):
        recs = np.array([c._record() for c in self.columns], dtype=np.int64).astype(np.int32).reshape(-1, 8)
        fracs = np.array([f for c in self.columns for f in c._fractions()], dtype=np.int64).astype(np.uint32).reshape(-1, 2)
        terms = np.array([t for c in self.columns for t in c._terms()], dtype=np.int64).astype(np.int32).reshape(-1, 4)
        if self.bend_records:
            self.bend_records(recs, fracs, terms)
        VP = ctypes.c_void_p
        L = self.pl.lib
        arg = lambda name, a: None if name in self.null or not a.size else a.ctypes.data
        return L.ms_build_logup_columns(self.pl.handle, self.base_field, self.ext_field, self.n,
                                        None if "base" in self.null else (VP * max(1, len(self.base_ptrs)))(*self.base_ptrs), len(self.base_ptrs),
                                        self.chal_ptr, self.nchal, arg("columns", recs), arg("fractions", fracs), arg("terms", terms), self.next,
                                        None if "outs" in self.null else (VP * max(1, len(self.out_ptrs)))(*self.out_ptrs))

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self):
        for o in self.outs:
            assert (o.to_numpy() == np.uint64(SENTINEL)).all()


def fresh(kind, pair_name="fp_fq3", n=300, columns=None):
    pl, pair = backends.planner(kind), PAIRS[pair_name]
    base, chal, designed, _ = case(pair_name, n, 10)
    d_base, d_chal = upload(pl, pair, base, chal)
    return Call(pl, pair, n, d_base, d_chal, designed[:3] if columns is None else columns)


ONE = [(+1, 0, 1)]


@pytest.mark.parametrize("kind", KINDS)
def test_too_many_fractions_terms_or_columns_are_unsupported(kind):
    nine = [(+1, 0, 1, 0)] * 9
    for columns in ([LogUpColumn(1, [(ONE, ONE)] * 5)], [LogUpColumn(1, [(ONE, ONE), (nine, ONE)])], [LogUpColumn(1, [(ONE, nine)])], [LogUpColumn(1, [(ONE, ONE)])] * 33):
        call = fresh(kind, columns=columns)
        assert call() == UNSUPPORTED, call.error()
        call.unchanged()
    ok = fresh(kind, columns=[LogUpColumn(1, [(nine[:8], nine[:8])] * 4)] * 32)          # the limits themselves are accepted
    assert ok() == 0, ok.error()


@pytest.mark.parametrize("kind", KINDS)
def test_indices_out_of_range_and_empty_denominators_are_refused(kind):
    frac = lambda num, den: LogUpColumn(1, [(ONE, ONE), (num, den)])
    bad = [frac([(+1, 0, NBASE)], ONE), frac(ONE, [(+1, 0, -2)]),                                                # a term's column
           frac([(+1, NCHAL, 0)], ONE), frac(ONE, [(-1, -2, 0)]),                                                # a term's challenge
           LogUpColumn(1, [(ONE, ONE)], mask=("nonzero", NBASE)), LogUpColumn(1, [(ONE, ONE)], mask=("zero", -1)),          # the mask's column
           LogUpColumn(("challenge", NCHAL), [(ONE, ONE)]), LogUpColumn(("challenge", -1), [(ONE, ONE)]),          # the init's challenge
           frac([(2, 0, 0)], ONE), frac(ONE, [(0, 0, 0)]),                                                       # a sign that is not +-1
           frac(ONE, []), frac([], [])]                                                                          # nd = 0
    for column in bad:
        call = fresh(kind, columns=[LogUpColumn(1, [(ONE, ONE)]), column])
        rc = call()
        assert rc == INVALID and any(word in call.error() for word in ("out of range", "sign", "nd = 0")), (rc, call.error())
        call.unchanged()


@pytest.mark.parametrize("kind", KINDS)
def test_unknown_init_and_mask_kinds_are_refused(kind):
    for word, value in ((0, 3), (0, -1), (2, 3), (2, -1)):                       # ms_logup_column.init, .mask
        call = fresh(kind)
        call.bend_records = lambda recs, fracs, terms, word=word, value=value: recs.__setitem__((1, word), value)
        assert call() == INVALID and "unknown" in call.error(), call.error()
        call.unchanged()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair_name", list(PAIRS))
def test_overlapping_outputs_are_refused(kind, pair_name):
    def refused(bend):
        call = fresh(kind, pair_name)
        bend(call)
        assert call() == INVALID and "overlap" in call.error(), call.error()
        call.unchanged()
    refused(lambda c: c.out_ptrs.__setitem__(1, c.base_ptrs[4]))              # a base column, referenced or not
    refused(lambda c: c.out_ptrs.__setitem__(0, c.base_ptrs[0] + 8))          # part of one
    refused(lambda c: c.out_ptrs.__setitem__(2, c.out_ptrs[0]))               # another output
    refused(lambda c: c.out_ptrs.__setitem__(2, c.out_ptrs[1] + 8 * (c.n - 1)))
    refused(lambda c: c.out_ptrs.__setitem__(1, c.chal_ptr))                  # the challenge vector


@pytest.mark.parametrize("kind", KINDS)
def test_null_arguments_and_unknown_field_pairs_are_refused(kind):
    for bend in (lambda c: setattr(c, "chal_ptr", None), lambda c: c.base_ptrs.__setitem__(2, None), lambda c: c.out_ptrs.__setitem__(1, None),
                 lambda c: setattr(c, "base_field", FQ3F), lambda c: setattr(c, "ext_field", F252F), lambda c: setattr(c, "base_field", F252F),
                 lambda c: setattr(c, "ext_field", 7), lambda c: setattr(c, "null", ("columns",)), lambda c: setattr(c, "null", ("fractions",)),
                 lambda c: setattr(c, "null", ("terms",)), lambda c: setattr(c, "null", ("base",)), lambda c: setattr(c, "null", ("outs",))):
        call = fresh(kind)
        bend(call)
        assert call() == INVALID, call.error()
        call.unchanged()
    call = fresh(kind)
    VP = ctypes.c_void_p
    assert call.pl.lib.ms_build_logup_columns(None, FP, FQ3F, call.n, (VP * NBASE)(*call.base_ptrs), NBASE, call.chal_ptr, NCHAL, None, None, None, 0,
                                              (VP * 1)(call.out_ptrs[0])) == INVALID
    call.unchanged()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair_name", list(PAIRS))
def test_checked_mode_refuses_non_canonical_input(kind, pair_name):
    pl, pair = backends.planner(kind), PAIRS[pair_name]
    n = 300
    base, chal, designed, want = case(pair_name, n, 10)
    p_words = [(pair.bf.p >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(pair.bf.nlimbs)]     # p itself: the smallest non-canonical value
    try:
        pl.checked(True)
        for where in ("base", "challenge"):
            bw = [pair.base_words(c) for c in base]
            cw = pair.ext_words(chal)
            if where == "base":
                bw[5][len(p_words) * 17:len(p_words) * 18] = p_words
            else:
                cw[-len(p_words):] = p_words                                                   # the last challenge (its last component)
            d_base = Matrix([GpuVec.from_numpy(pl, w, pair.base_field) for w in bw])
            d_chal = GpuVec.from_numpy(pl, cw, pair.ext_field)
            call = Call(pl, pair, n, d_base, d_chal, designed)
            assert call() == INVALID, call.error()
            msg = call.error()
            assert "canonical" in msg and "ms_build_logup_columns" in msg and ("d_base" if where == "base" else "d_challenges") in msg, msg
            call.unchanged()
        # canonical input passes under the mode, with the same words
        d_base, d_chal = upload(pl, pair, base, chal)
        got = build_logup_columns(pl, d_base, d_chal, designed, pair.ext_field)
        assert all(np.array_equal(g, pair.ext_words(w)) for g, w in zip(got.to_numpy(), want))
    finally:
        pl.checked(False)


def test_python_mirror_raises_with_the_library_message():
    pl, pair = backends.planner("emu"), PAIRS["fp_fp"]
    base, chal, _, _ = case("fp_fp", 3, 10)
    d_base, d_chal = upload(pl, pair, base, chal)
    with pytest.raises(MsError) as err:
        build_logup_columns(pl, d_base, d_chal, [LogUpColumn(1, [(ONE, [(+1, 0, 99)])])], FP)
    assert err.value.code == INVALID and "out of range" in str(err.value)
    with pytest.raises(MsError) as err:
        build_extension_columns(pl, d_base, d_chal, [LogUpColumn(1, [(ONE, [])])], FP)
    assert err.value.code == INVALID and "nd = 0" in str(err.value)
    with pytest.raises(ValueError):
        build_logup_columns(pl, d_base, d_chal, [LogUpColumn(2, [])], FP)
    with pytest.raises(ValueError):
        build_logup_columns(pl, d_base, d_chal, [], FQ3F)                      # the challenges are Fp elements
    with pytest.raises(TypeError):
        build_logup_columns(pl, d_base, d_chal, [extension.ExtColumn(1, [], [])], FP)
