"""ms_build_extension_columns (include/ministark_hip_ext.h; Trace::build_extension_columns, examples/brainfuck/trace.rs:108-289) against
the sequential loop on Python integers (tests/ext_ref.py), word for word: lengths around the rows of a workgroup, offsets that wrap, 0 / 1 /
8 terms per map, literal-1 coefficients, both signs, the three inits, the three masks, inclusive and exclusive output, 1 / 9 / 32 columns
in a call, the three field pairs -- and the refusals, after which the sentinel-filled outputs are unchanged.  The kernels have ONE
instantiation per field pair (4 rows per lane at every length), so the tile has no long-column case; the walk of the block aggregates has:
ext_blocks is one workgroup per column whose lane t walks ceil(nblocks / 256) blocks, one block each up to 256 blocks = 256 * ROWS rows, two
from the next row on.  test_block_walk_past_256_blocks runs both sides of that edge."""
import ctypes
import functools

import numpy as np
import pytest

from tests import backends
from tests.ext_ref import PAIRS, reference
from ministark_amd import ExtColumn, GpuVec, Matrix, build_extension_columns, extension
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, STARK252_FP as F252F
from ministark_amd._lib import MsError

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
B = extension.ROWS_PER_WORKGROUP           # msext::ROWS, the rows per workgroup (tests/test_ext_abi.py checks it against ext_kernels.h)
LENGTHS = [1, 2, 3, 255, 256, 1023, 1024, 1025, 2 * B + 1]
NBASE, NCHAL = 9, 5                       # base columns 0..5 random, 6 a random 0 / non-zero mix, 7 all zero, 8 zero but for the last row
INVALID, UNSUPPORTED = -1, -2


def offsets(n):
    return [0, 1, -1, n - 1, -n - 1, 5 * n + 2]


def designed_columns(n):
    """nine columns that between them take every path the header describes"""
    o = offsets(n)
    eight = lambda s: [((+1, -1)[(k + s) % 2], (None, 0, 1, 2, 3, 4)[(k + s) % 6], (None, 0, 1, 2, 3, 4, 5)[(3 * k + s) % 7], o[(k + s) % 6]) for k in range(8)]
    return [
        ExtColumn(1, [(+1, 0, None), (-1, 1, 0, 0), (-1, 2, 1, 1)], [], mask=("nonzero", 6)),                  # a masked running product
        ExtColumn(0, [(+1, 3, None)], [(+1, None, 2, 1)], inclusive=True),                                      # a running evaluation, +1 row offset
        ExtColumn(("challenge", 1), [], eight(0), mask=("zero", 6)),                                            # empty A, 8 terms in B
        ExtColumn(("challenge", 0), eight(1), eight(2), inclusive=True),                                        # 8 and 8
        ExtColumn(1, [], []),                                                                                   # no term at all: the init everywhere
        ExtColumn(("challenge", 4), [(-1, None, 3, -1)], [(-1, 2, None)], mask=("nonzero", 7)),                 # inactive everywhere
        ExtColumn(1, [(+1, 0, 4, n - 1)], [(+1, 1, 5, -n - 1)], mask=("nonzero", 8), inclusive=True),           # active on the last row only
        ExtColumn(0, [(-1, None, 4, 5 * n + 2)], [(+1, 3, 5, 5 * n + 2)], mask=("zero", 7)),                    # a mask that is active everywhere
        ExtColumn(0, [(+1, None, None)], [(+1, None, None), (-1, None, 0, 2)]),                                 # constants with the literal 1
    ]


def random_columns(rng, n, count):
    o = offsets(n)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    term = lambda: (pick((+1, -1)), pick((None,) + tuple(range(NCHAL))), pick((None,) + tuple(range(NBASE))), pick(o))
    out = []
    for _ in range(count):
        out.append(ExtColumn(pick((0, 1, ("challenge", pick(range(NCHAL))))), [term() for _ in range(pick((0, 1, 3, 8)))],
                             [term() for _ in range(pick((0, 1, 2, 8)))], mask=pick((None, ("nonzero", 6), ("zero", 6), ("nonzero", 8))),
                             inclusive=pick((False, True))))
    return out


@functools.lru_cache(maxsize=None)
def case(pair_name, n, count):
    """(base columns, challenges, column records, expected values), computed once and shared by the backends"""
    pair = PAIRS[pair_name]
    rng = np.random.default_rng(1000 * n + count)
    base = [pair.random_base(rng, n) for _ in range(6)]
    base.append([v if k else 0 for v, k in zip(pair.random_base(rng, n), rng.integers(0, 3, size=n))])
    base.append([0] * n)
    base.append([0] * (n - 1) + [7])
    chal = pair.random_ext(rng, NCHAL)
    columns = designed_columns(n) if count == 9 else random_columns(rng, n, count)
    return base, chal, columns, reference(pair, base, chal, columns)


def upload(pl, pair, base, chal):
    return (Matrix([GpuVec.from_numpy(pl, pair.base_words(c), pair.base_field) for c in base]),
            GpuVec.from_numpy(pl, pair.ext_words(chal), pair.ext_field))


def run_case(kind, pair_name, n, count):
    pl, pair = backends.planner(kind), PAIRS[pair_name]
    base, chal, columns, want = case(pair_name, n, count)
    d_base, d_chal = upload(pl, pair, base, chal)
    got = build_extension_columns(pl, d_base, d_chal, columns, pair.ext_field)
    assert got.num_cols() == count and got.field == pair.ext_field
    for e, (g, w) in enumerate(zip(got.to_numpy(), want)):
        assert np.array_equal(g, pair.ext_words(w)), (pair_name, n, e)
    for c, v in zip(d_base.columns, base):                                    # the inputs are only read
        assert np.array_equal(c.to_numpy(), pair.base_words(v))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair_name", list(PAIRS))
@pytest.mark.parametrize("n", LENGTHS)
def test_nine_designed_columns(kind, pair_name, n):
    run_case(kind, pair_name, n, 9)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair_name", list(PAIRS))
@pytest.mark.parametrize("count", [1, 32])
def test_batch_shapes(kind, pair_name, count):
    run_case(kind, pair_name, 1025, count)


# ---- the block walk: 256 blocks (one per lane of ext_blocks) and 257 (two per lane, lane 128 holds the last one) ------------------------
WALK_LENGTHS = [256 * B, 256 * B + 1]
WALK_GUARD = np.array([0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A] * 8, dtype=np.uint64)


def walk_columns():
    """three light columns in one call (gridDim.y = 3: every column has its own slice of agg and block_state); at most two terms per map,
    the reference being a Python loop.  Base columns: 0, 1 values; 2 the mask of the first column (zero on row 0, non-zero on the last rows);
    3 the mask of the third (non-zero on row 0, zero on the last rows)."""
    return [
        ExtColumn(1, [(+1, 0, None), (-1, None, 0, -1)], [], mask=("nonzero", 2)),                             # a masked running product of (chal0 - col0[i-1])
        ExtColumn(0, [(+1, 1, None)], [(+1, 2, 1, +1)], inclusive=True),                                        # a running evaluation state * chal1 + chal2 * col1[i+1]
        ExtColumn(("challenge", 3), [(+1, 4, 1)], [(+1, None, 0), (-1, 2, None)], mask=("zero", 3)),            # a challenge init under an if-zero mask
    ]


def walk_words(pair, vals, cubic=False):
    """pair.base_words / pair.ext_words for a quarter of a million values: one list comprehension, the limbs cut from bytes"""
    flat = [c for v in vals for c in v] if cubic else vals
    R, p = pair.bf.R, pair.bf.p
    raw = b"".join(((x * R) % p).to_bytes(pair.bf.nbytes, "little") for x in flat)
    return np.frombuffer(raw, dtype=np.uint64).copy()


@functools.lru_cache(maxsize=None)
def walk_case(pair_name, n):
    """(base columns, challenges, column records, base words, challenge words, expected words), computed once and shared by the backends"""
    pair = PAIRS[pair_name]
    rng = np.random.default_rng(77 + n)

    def values():
        if pair.bf.nlimbs == 1:
            return rng.integers(0, pair.bf.p, size=n, dtype=np.uint64).tolist()
        limbs = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        limbs[:, 3] >>= np.uint64(5)                      # below 2^251 < p
        raw = limbs.tobytes()
        return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    base = [values(), values()]
    keep = rng.integers(0, 3, size=n)
    keep[0], keep[-(B + 3):] = 0, 1                      # the first column: inactive on row 0, active on every row of the last block (and on the block before it)
    base.append([v if k else 0 for v, k in zip(values(), keep)])
    base.append([0 if k else v + 1 if v + 1 < pair.bf.p else 1 for v, k in zip(base[2], keep)])          # zero exactly where column 2 is not
    chal = pair.random_ext(rng, NCHAL)
    columns = walk_columns()
    assert base[2][0] == 0 and base[3][0] != 0 and all(base[2][-B:]) and not any(base[3][-B:])
    assert 0 in base[2][B:-B - 3] and 0 in base[3][B:-B - 3]                                                 # both masks switch in the middle blocks too
    want = reference(pair, base, chal, columns)
    for vals in (base[0][:40], base[2][-40:]):
        assert np.array_equal(walk_words(pair, vals), pair.base_words(vals))
    assert np.array_equal(walk_words(pair, want[1][-40:], pair.cubic), pair.ext_words(want[1][-40:]))
    return base, chal, columns, [walk_words(pair, c) for c in base], pair.ext_words(chal), [walk_words(pair, w, pair.cubic) for w in want]


# the simulator takes the longer length (two blocks per lane) only: it needs seconds for a quarter of a million rows of three columns
@pytest.mark.parametrize("kind,n", [pytest.param(kind, n, id=f"{n}-{kind}", marks=[pytest.mark.gpu] if kind == "hip" else [])
                                    for n in WALK_LENGTHS for kind in ("emu", "hip") if kind == "hip" or n == WALK_LENGTHS[1]])
@pytest.mark.parametrize("pair_name", list(PAIRS))
def test_block_walk_past_256_blocks(kind, pair_name, n):
    """raw call: every output has guard words behind its last element; the base columns and the challenges are compared after it"""
    pl, pair = backends.planner(kind), PAIRS[pair_name]
    assert -(-n // B) == (256 if n == 256 * B else 257)
    base, chal, columns, base_w, chal_w, want_w = walk_case(pair_name, n)
    d_base = Matrix([GpuVec.from_numpy(pl, w, pair.base_field) for w in base_w])
    d_chal = GpuVec.from_numpy(pl, chal_w, pair.ext_field)
    call = Call(pl, pair, n, d_base, d_chal, columns)
    V = {FP: 1, FQ3F: 3, F252F: 4}[pair.ext_field]
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
    base, chal, columns, _ = case("fp_fq3", 3, 9)
    d_base, d_chal = upload(pl, pair, base, chal)
    assert build_extension_columns(pl, d_base, d_chal, [], FQ3F).num_cols() == 0
    call = Call(pl, pair, 3, d_base, d_chal, columns[:2])
    call.n = 0
    assert call() == 0
    call.unchanged()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5A5A5A5A5A5A5A5


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

    def __call__(self):
        recs = np.array([c._record() for c in self.columns], dtype=np.int64).astype(np.int32)
        terms = np.array([t for c in self.columns for t in c._terms()], dtype=np.int64).astype(np.int32).reshape(-1, 4)
        VP = ctypes.c_void_p
        L = self.pl.lib
        return L.ms_build_extension_columns(self.pl.handle, self.base_field, self.ext_field, self.n, (VP * max(1, len(self.base_ptrs)))(*self.base_ptrs),
                                            len(self.base_ptrs), self.chal_ptr, self.nchal, recs.ctypes.data, terms.ctypes.data if terms.size else None,
                                            len(self.columns), (VP * max(1, len(self.out_ptrs)))(*self.out_ptrs))

    def error(self):
        return self.pl.lib.ms_last_error().decode()

    def unchanged(self):
        for o in self.outs:
            assert (o.to_numpy() == np.uint64(SENTINEL)).all()


def fresh(kind, pair_name="fp_fq3", n=300, columns=None):
    pl, pair = backends.planner(kind), PAIRS[pair_name]
    base, chal, designed, _ = case(pair_name, n, 9)
    d_base, d_chal = upload(pl, pair, base, chal)
    return Call(pl, pair, n, d_base, d_chal, designed[:3] if columns is None else columns)


@pytest.mark.parametrize("kind", KINDS)
def test_too_many_terms_or_columns_are_unsupported(kind):
    nine = [(+1, 0, 1, 0)] * 9
    for columns in ([ExtColumn(1, nine, [])], [ExtColumn(1, [], nine)], [ExtColumn(1, [(+1, 0, 1)], [])] * 33):
        call = fresh(kind, columns=columns)
        assert call() == UNSUPPORTED, call.error()
        call.unchanged()
    ok = fresh(kind, columns=[ExtColumn(1, nine[:8], nine[:8])] * 32)          # the limits themselves are accepted
    assert ok() == 0, ok.error()


@pytest.mark.parametrize("kind", KINDS)
def test_indices_out_of_range_are_refused(kind):
    bad = [ExtColumn(1, [(+1, 0, NBASE)], []), ExtColumn(1, [], [(+1, 0, -2)]),                      # a term's column
           ExtColumn(1, [(+1, NCHAL, 0)], []), ExtColumn(1, [], [(-1, -2, 0)]),                       # a term's challenge
           ExtColumn(1, [(+1, 0, 0)], [], mask=("nonzero", NBASE)), ExtColumn(1, [(+1, 0, 0)], [], mask=("zero", -1)),       # the mask's column
           ExtColumn(("challenge", NCHAL), [(+1, 0, 0)], []), ExtColumn(("challenge", -1), [(+1, 0, 0)], []),              # the init's challenge
           ExtColumn(1, [(2, 0, 0)], [])]                                                             # a sign that is not +-1
    for column in bad:
        call = fresh(kind, columns=[ExtColumn(1, [(+1, 0, 0)], []), column])
        rc = call()
        assert rc == INVALID and ("out of range" in call.error() or "sign" in call.error()), (rc, call.error())
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
def test_null_tables_and_unknown_field_pairs_are_refused(kind):
    for bend in (lambda c: setattr(c, "chal_ptr", None), lambda c: c.base_ptrs.__setitem__(2, None), lambda c: c.out_ptrs.__setitem__(1, None),
                 lambda c: setattr(c, "base_field", FQ3F), lambda c: setattr(c, "ext_field", F252F), lambda c: setattr(c, "base_field", F252F),
                 lambda c: setattr(c, "ext_field", 7)):
        call = fresh(kind)
        bend(call)
        assert call() == INVALID, call.error()
        call.unchanged()
    call = fresh(kind)
    L, VP = call.pl.lib, ctypes.c_void_p
    recs = np.zeros((1, 8), dtype=np.int32)
    outs = (VP * 1)(call.out_ptrs[0])
    assert L.ms_build_extension_columns(call.pl.handle, FP, FQ3F, call.n, None, NBASE, call.chal_ptr, NCHAL, recs.ctypes.data, None, 1, outs) == INVALID
    assert L.ms_build_extension_columns(call.pl.handle, FP, FQ3F, call.n, (VP * NBASE)(*call.base_ptrs), NBASE, call.chal_ptr, NCHAL, None, None, 1, outs) == INVALID
    assert L.ms_build_extension_columns(call.pl.handle, FP, FQ3F, call.n, (VP * NBASE)(*call.base_ptrs), NBASE, call.chal_ptr, NCHAL, recs.ctypes.data, None, 1, None) == INVALID
    call.unchanged()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair_name", list(PAIRS))
def test_checked_mode_refuses_non_canonical_input(kind, pair_name):
    pl, pair = backends.planner(kind), PAIRS[pair_name]
    n = 300
    base, chal, designed, want = case(pair_name, n, 9)
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
            assert "canonical" in msg and "ms_build_extension_columns" in msg and ("d_base" if where == "base" else "d_challenges") in msg, msg
            call.unchanged()
        # canonical input passes under the mode, with the same words
        d_base, d_chal = upload(pl, pair, base, chal)
        got = build_extension_columns(pl, d_base, d_chal, designed, pair.ext_field)
        assert all(np.array_equal(g, pair.ext_words(w)) for g, w in zip(got.to_numpy(), want))
    finally:
        pl.checked(False)


def test_python_mirror_raises_with_the_library_message():
    pl, pair = backends.planner("emu"), PAIRS["fp_fp"]
    base, chal, _, _ = case("fp_fp", 3, 9)
    d_base, d_chal = upload(pl, pair, base, chal)
    with pytest.raises(MsError) as err:
        build_extension_columns(pl, d_base, d_chal, [ExtColumn(1, [(+1, 0, 99)], [])], FP)
    assert err.value.code == INVALID and "out of range" in str(err.value)
    with pytest.raises(ValueError):
        build_extension_columns(pl, d_base, d_chal, [ExtColumn(2, [], [])], FP)
    with pytest.raises(ValueError):
        build_extension_columns(pl, d_base, d_chal, [], FQ3F)                  # the challenges are Fp elements
