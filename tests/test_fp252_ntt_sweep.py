"""Sweep of the 252-bit transforms through the C ABI: ms_ntt_enqueue / ms_ntt_enqueue_to, ms_lde and ms_evaluate on Fp252 columns, at the sizes,
values, batch widths and blow-ups where csrc/ms_ntt252.cpp and csrc/ms_ntt.cpp change route and where the lazily reduced tiles of csrc/fp252_ntt_kernels.h could
come out wrong.  Every output word is compared with the C oracle (oracle.cref.ntt252 / lde252 / bit_reverse, pinned to the big-integer
restatement by tests/test_fp252_parity.py::test_c_oracle_ntt_252_matches_bigint), bit for bit; the zero and the constant columns also with
their closed forms, which need no oracle.

The routes (plan_run252 in ms_ntt252.cpp, the plans of plan_build252 in ms_ntt_plan.cpp, ms_lde / ms_evaluate in ms_ntt.cpp).  Below 2^11 points a column is bit-reversed, transformed by ntt252_local (up to 2^9 points in LDS) and, above 2^9,
by ntt252_stages, one column per launch, through a device copy when the transform is out of place (plan_run252).  From 2^11 points on the tiled
passes run (plan_run252_tiled): two passes up to 2^20 points, three above (MS_NTT252_PASSES=3: from 2^17 on), with the radices
lr252 = log_n split evenly, the larger ones first -- (6, 5) at 2^11, (6, 6) at 2^12, (7, 6) at 2^13, (6, 6, 5) at a three-pass 2^17, (9, 9) at
2^18.  Pass 1 reads src[c], the passes between work in scratch, the last pass writes dst[c]; a call's columns go in groups of
min(256, MS_NTT_GROUP_BYTES / column bytes) per launch.  ms_lde and ms_evaluate hand the zero extension to pass 1 (only 2^lr0 >> log_blowup rows
of a tile are read) and the bit reversal to the last pass while log_blowup <= lr0; beyond that they fill the padding, transform the whole
domain and bit-reverse on their own.

The values.  A tile keeps residues unreduced (X + T, X + (K p - T), below 24 p < 2^256) and reduces once at the end, so a zero column travels as
2p, 4p, ... and a constant column cancels to exact multiples of p everywhere but at one output: those are the inputs that ask whether k p
comes back as the word 0.  The columns here hold the words the kernels read (Montgomery representatives); `p - 1` is the largest canonical
word."""
import contextlib

import numpy as np
import pytest

from oracle import cref
from oracle.pyref import fields as PF
from tests import backends
from tests.test_fp252_parity import DIGIT_EDGES_252
from ministark_amd import (STARK252_FP, GpuFft, GpuIfft, GpuVec, Matrix, Planner, Radix2EvaluationDomain, f252_to_mont_limbs)

P = PF.F252_P
TILE_LOG = 11                              # ms252::TILE_LOG: from 2^11 points on the tiled passes run
LOCAL_LOG = 9                              # ms252::CHUNK_LOG: what ntt252_local transforms on its own
DIRECTIONS = [(False, 1), (False, 3), (True, 1), (True, 3)]          # (inverse, coset offset); 3 is the field's generator


def _params(emu, hip):
    """(kind, log_n) for every size of `emu` on the simulator and every size of `hip` on the device"""
    return [pytest.param("emu", n, id=f"emu-{n}") for n in emu] + [pytest.param("hip", n, id=f"hip-{n}", marks=pytest.mark.gpu) for n in hip]


KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


def words(v):
    """the four little-endian words of an integer below 2^256"""
    return np.array([(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


def rand_col(log_n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 59, size=4 << log_n, dtype=np.uint64)      # limbs < 2^59: canonical (< p)


class Oracle:
    """cref.ntt252 of a batch, one call per distinct column content"""

    def __init__(self):
        self.memo = {}

    def ntt(self, x, log_n, inverse, offset):
        key = (x.tobytes(), log_n, inverse, offset)
        if key not in self.memo:
            self.memo[key] = cref.ntt252(x, log_n, inverse, f252_to_mont_limbs(offset))
        return self.memo[key]


def plan_for(pl, log_n, inverse, offset):
    return (GpuIfft if inverse else GpuFft)(Radix2EvaluationDomain(1 << log_n, offset, STARK252_FP), STARK252_FP, pl)


def upload(pl, cols):
    return [GpuVec.from_numpy(pl, c, STARK252_FP) for c in cols]


def blank(pl, cols):
    return [GpuVec(pl, c.size // 4, STARK252_FP) for c in cols]


def expected_route(log_n, passes=None):
    if log_n < TILE_LOG:
        return {"ntt252_local"} | ({"ntt252_stages"} if log_n > LOCAL_LOG else set())
    passes = passes or (2 if log_n <= 20 else 3)
    return {"ntt252_pass1", "ntt252_pass2", "ntt252_pass3"} if passes == 3 else {"ntt252_pass1", "ntt252_pass2"}


@contextlib.contextmanager
def profiled(pl):
    """-> a dict filled, when the block ends, with {kernel: launches} of what ran inside it"""
    calls = {}
    pl.profile(True)
    try:
        yield calls
        calls.update({k: v["calls"] for k, v in pl.profile_read().items()})
    finally:
        pl.profile(False)


@contextlib.contextmanager
def fresh_planner(kind, monkeypatch, **env):
    """A context of its own with `env` set: MS_NTT_GROUP_BYTES is read when a context is created, MS_NTT252_PASSES when a plan is built, and the
    plan cache belongs to the context -- the shared planner would hand back whatever plan the process built before.  Columns allocated through
    `keep` are released before the context is."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    pl = Planner(0, backends.planner(kind).lib)
    keep = []
    try:
        yield pl, keep
    finally:
        for v in keep:
            v.free()
        pl.close()


def both_ways(pl, cols, log_n, inverse, offset, oracle, passes=None):
    """dst = transform(src) out of place (every source word kept), then the same columns in place and one call whose dst IS its src; the
    kernels that ran are those of the size's route.  -> the columns' transforms"""
    src, dst, alias = upload(pl, cols), blank(pl, cols), upload(pl, cols[:1])
    plan = plan_for(pl, log_n, inverse, offset)
    with profiled(pl) as calls:
        plan.enqueue_to(src, dst)
        kept = [s.to_numpy() for s in src]
        plan.enqueue(src)
        plan.enqueue_to(alias, alias)
    plan.close()
    assert set(calls) == expected_route(log_n, passes), (calls, log_n)
    want = [oracle.ntt(c, log_n, inverse, offset) for c in cols]
    for i, (c, k, s, d, w) in enumerate(zip(cols, kept, src, dst, want)):
        assert np.array_equal(k, c), f"column {i}: the source of the out-of-place transform changed"
        assert np.array_equal(d.to_numpy(), w), f"column {i} out of place (log_n={log_n} inverse={inverse} offset={offset})"
        assert np.array_equal(s.to_numpy(), w), f"column {i} in place (log_n={log_n} inverse={inverse} offset={offset})"
    assert np.array_equal(alias[0].to_numpy(), want[0]), "dst == src"
    return want


# ------------------------------------------------------------------------------------------------------------------
# 1. every size, a batch of three, both directions
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log_n", _params(range(0, 14), range(0, 19)))
def test_every_size_three_columns_both_ways(kind, log_n):
    """2^0 .. 2^18 points (the simulator: up to 2^13): three distinct random columns, forward and inverse, subgroup and coset.  Covers the path
    below 2^11 at every size (no stage at all at 2^0, ntt252_local alone up to 2^9, then one more stage in ntt252_stages at 2^10) and every
    two-pass split from (6, 5) to (9, 9), the odd radices with the lone last stage of tile_dit among them."""
    pl = backends.planner(kind)
    cols = [rand_col(log_n, 100 * log_n + c) for c in range(3)]
    oracle = Oracle()
    for inverse, offset in DIRECTIONS:
        both_ways(pl, cols, log_n, inverse, offset, oracle)


@pytest.mark.gpu
def test_three_real_passes_two_columns_out_of_place_hip():
    """2^21 points: (7, 7, 7), pass 2 in scratch between a pass that reads src and one that writes dst"""
    pl = backends.planner("hip")
    both_ways(pl, [rand_col(21, 2100 + c) for c in range(2)], 21, False, 3, Oracle())


@pytest.mark.gpu
def test_inverse_coset_scale_table_past_its_split_hip():
    """2^22 points, inverse on the coset: the last pass multiplies output k by n^-1 h^-k from the two-level table, whose high half is first
    read at k = 2^21"""
    pl = backends.planner("hip")
    x = rand_col(22, 2200)
    src, dst = upload(pl, [x]), blank(pl, [x])
    plan = plan_for(pl, 22, True, 3)
    with profiled(pl) as calls:
        plan.enqueue_to(src, dst)
    plan.close()
    assert set(calls) == expected_route(22), calls
    assert np.array_equal(src[0].to_numpy(), x)
    assert np.array_equal(dst[0].to_numpy(), cref.ntt252(x, 22, True, f252_to_mont_limbs(3)))


@pytest.mark.parametrize("kind", KINDS)
def test_matrix_interpolate_and_evaluate(kind):
    """Matrix.interpolate / Matrix.evaluate on a domain of the columns' size: new columns through ms_ntt_enqueue_to, the matrix itself kept"""
    pl = backends.planner(kind)
    log_n = 12
    cols = [rand_col(log_n, 1200 + c) for c in range(3)]
    m = Matrix(upload(pl, cols))
    for offset in (1, 3):
        dom = Radix2EvaluationDomain(1 << log_n, offset, STARK252_FP)
        off = f252_to_mont_limbs(offset)
        polys, evals = m.interpolate(dom), m.evaluate(dom)
        for c, k, a, b in zip(cols, m.to_numpy(), polys.to_numpy(), evals.to_numpy()):
            assert np.array_equal(k, c), "the matrix must keep its columns"
            assert np.array_equal(a, cref.ntt252(c, log_n, True, off)), offset
            assert np.array_equal(b, cref.ntt252(c, log_n, False, off)), offset


# ------------------------------------------------------------------------------------------------------------------
# 2. structured columns: exact multiples of p inside the tiles
# ------------------------------------------------------------------------------------------------------------------
CONST = 0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_8796A5B4C3D2E1F0 % P      # "a constant c": any word with no structure of its own
PATTERNS = ["zero", "all_pm1", "const", "alternating", "pm1_last", "pm1_first", "digit_edges"]


def structured(pattern, log_n):
    n = 1 << log_n
    a = np.zeros((n, 4), dtype=np.uint64)
    if pattern == "all_pm1":
        a[:] = words(P - 1)
    elif pattern == "const":
        a[:] = words(CONST)
    elif pattern == "alternating":                       # 0, p - 1, 0, p - 1, ...
        a[1::2] = words(P - 1)
    elif pattern == "pm1_last":
        a[n - 1] = words(P - 1)
    elif pattern == "pm1_first":
        a[0] = words(P - 1)
    elif pattern == "digit_edges":                       # the list in order, then drawn from it: raw words, all canonical
        edge = np.array([words(v % P) for v in DIGIT_EDGES_252])
        pick = np.random.default_rng(17).integers(0, len(edge), size=n)
        pick[:len(edge)] = np.arange(len(edge))[:n]
        a[:] = edge[pick]
    else:
        assert pattern == "zero", pattern
    return a.reshape(-1)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind,log_n", _params([0, 1, 2, 3, 8, 10, 11, 12, 13], [0, 1, 2, 3, 8, 10, 11, 12, 13, 16, 17, 18]))
def test_structured_columns(kind, log_n, pattern):
    """Zero, p - 1 everywhere, a constant, 0 / p - 1 alternating, a lone p - 1 at either end, and the digit-edge words: forward and inverse,
    subgroup and coset, in place and out of place, against the oracle.  On the subgroup the zero and the constant column are also held
    against what they must give whatever the oracle says: zero gives zero; a constant c gives n c at index 0 and the WORD 0 at every other
    output (each of them a multiple of p inside the tile); and the inverse of that brings c back everywhere."""
    pl = backends.planner(kind)
    n = 1 << log_n
    x = structured(pattern, log_n)
    oracle = Oracle()
    for inverse, offset in DIRECTIONS:
        got = both_ways(pl, [x], log_n, inverse, offset, oracle)[0]           # == the device's output, word for word
        if pattern == "zero":
            assert not got.any(), (inverse, offset)
        if pattern == "const" and offset == 1 and not inverse:
            closed = np.zeros((n, 4), dtype=np.uint64)
            closed[0] = words(n * CONST % P)
            assert np.array_equal(got, closed.reshape(-1)), "forward transform of a constant column"
            back = both_ways(pl, [got], log_n, True, 1, oracle)[0]
            assert np.array_equal(back, x), "inverse transform of n c, 0, 0, ..."


# ------------------------------------------------------------------------------------------------------------------
# 3. more columns than a launch takes, and groups smaller than the batch
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log_n", [9, 11])
def test_batch_wider_than_a_launch(kind, log_n):
    """259 columns in one call: 256 + 3 on the tiled route (msntt::MAXC columns per launch, the second group starts at c0 = 256), one column
    after another below it.  Three contents in turn (column 256 holds another one than column 0), so that a column skipped, read from or written to
    another one's place shows; out of place, every source kept."""
    pl = backends.planner(kind)
    ncols = 259
    contents = [rand_col(log_n, 300 + log_n + c) for c in range(3)]
    cols = [contents[c % 3] for c in range(ncols)]
    src, dst = upload(pl, cols), blank(pl, cols)
    oracle = Oracle()
    fwd = plan_for(pl, log_n, False, 3)
    with profiled(pl) as calls:
        fwd.enqueue_to(src, dst)
    fwd.close()
    assert set(calls) == expected_route(log_n), calls
    if log_n >= TILE_LOG:
        assert calls == {"ntt252_pass1": 2, "ntt252_pass2": 2}, calls
    else:
        assert calls == {"ntt252_local": ncols}, calls
    for i, (c, s, d) in enumerate(zip(cols, src, dst)):
        assert np.array_equal(s.to_numpy(), c), f"source column {i}"
        assert np.array_equal(d.to_numpy(), oracle.ntt(c, log_n, False, 3)), f"column {i}"
    assert len(oracle.memo) == 3
    for v in src + dst:
        v.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inverse", [False, True])
def test_split_groups_three_passes(kind, inverse, monkeypatch):
    """Five columns of 2^17 points with room for two per group and the three-pass split forced: groups of 2 + 2 + 1, each restarting at its
    c0 for the sources of pass 1 and the destinations of pass 3, with pass 2 in the scratch of the group.  Out of place, forward and inverse,
    one column all zero."""
    log_n, ncols = 17, 5
    with fresh_planner(kind, monkeypatch, MS_NTT_GROUP_BYTES=2 * (32 << log_n), MS_NTT252_PASSES=3) as (pl, keep):
        cols = [rand_col(log_n, 1700 + c) for c in range(ncols)]
        cols[3] = np.zeros(4 << log_n, dtype=np.uint64)
        src, dst = upload(pl, cols), blank(pl, cols)
        keep += src + dst
        plan = plan_for(pl, log_n, inverse, 3)
        with profiled(pl) as calls:
            plan.enqueue_to(src, dst)
        plan.close()
        assert calls == {"ntt252_pass1": 3, "ntt252_pass2": 3, "ntt252_pass3": 3}, calls
        for i, (c, s, d) in enumerate(zip(cols, src, dst)):
            assert np.array_equal(s.to_numpy(), c), f"source column {i}"
            assert np.array_equal(d.to_numpy(), cref.ntt252(c, log_n, inverse, f252_to_mont_limbs(3))), f"column {i}"
        assert not dst[3].to_numpy().any()


# ------------------------------------------------------------------------------------------------------------------
# 4. LDE and evaluate where the zero extension meets the first radix
# ------------------------------------------------------------------------------------------------------------------
def first_radix(log_N, passes=None):
    """lr252[0] of the plan of a 2^log_N domain (None: not a tiled domain)"""
    if log_N < TILE_LOG:
        return None
    passes = passes or (2 if log_N <= 20 else 3)
    return -(-log_N // passes)


OPS = ("lde_bit_reversed", "lde_natural", "evaluate", "bit_reversed_evaluate")


def lde_and_evaluate(pl, log_n, log_b, offset, ncols, passes=None, keep=None, ops=OPS):
    """Matrix.lde in both output orders and evaluate / bit_reversed_evaluate of the same columns read as coefficients, on the domain of
    2^(log_n + log_b) points; every input word kept.  While log_b <= lr0 the forward half must be the tiled passes alone, one launch each."""
    log_N = log_n + log_b
    off = f252_to_mont_limbs(offset)
    cols = [rand_col(log_n, 4000 + 64 * log_n + 4 * log_b + c) for c in range(ncols)]
    vecs = upload(pl, cols)
    m = Matrix(vecs)
    dom = Radix2EvaluationDomain(1 << log_N, offset, STARK252_FP)
    lr0 = first_radix(log_N, passes)
    forward_half = expected_route(log_N, passes)
    evaluations = {}

    def evaluation(c):                                    # of column c's coefficients, natural order
        if c not in evaluations:
            padded = np.concatenate([cols[c], np.zeros((4 << log_N) - cols[c].size, dtype=np.uint64)])
            evaluations[c] = cref.ntt252(padded, log_N, False, off)
        return evaluations[c]
    want = {"lde_bit_reversed": lambda c: cref.lde252(cols[c], log_n, log_b, off, True),
            "lde_natural": lambda c: cref.lde252(cols[c], log_n, log_b, off, False),
            "evaluate": evaluation,
            "bit_reversed_evaluate": lambda c: cref.bit_reverse(evaluation(c), log_N, 4)}
    for op in ops:
        with profiled(pl) as calls:
            out = {"lde_bit_reversed": lambda: m.lde(1 << log_b, offset, True), "lde_natural": lambda: m.lde(1 << log_b, offset, False),
                   "evaluate": lambda: m.evaluate(dom), "bit_reversed_evaluate": lambda: m.bit_reversed_evaluate(dom)}[op]()
        if keep is not None:
            keep += out.columns
        if lr0 is not None:
            inverse_half = expected_route(log_n, passes if log_n >= 17 else None) if op.startswith("lde") else set()
            assert set(calls) == forward_half | inverse_half, (op, calls)
            if log_b <= lr0:                              # fused: nothing but one launch of each pass
                assert all(calls[k] == (2 if k in inverse_half else 1) for k in forward_half), (op, calls)
        for c in range(ncols):
            assert np.array_equal(out.columns[c].to_numpy(), want[op](c)), f"{op}, column {c}"
            assert np.array_equal(vecs[c].to_numpy(), cols[c]), f"{op} changed input column {c}"
        if keep is None:
            for v in out.columns:
                v.free()
    if keep is None:
        for v in vecs:
            v.free()
    else:
        keep += vecs


# (log_n, log_b) -> domain 2^(log_n + log_b); lr0 = 6 at 2^11 and 2^12, 7 at 2^13.  Around log_b == lr0: one row of the tile holds
# coefficients at log_b == lr0, beyond it the padding is written out and the whole domain transformed
LDE_PAIRS = [(11, 0), (10, 1), (6, 5), (5, 6), (4, 7),                       # 2^11: fused up to log_b = 6
             (12, 0), (11, 1), (7, 5), (6, 6), (5, 7), (1, 11),              # 2^12: fused up to log_b = 6
             (7, 6), (6, 7), (5, 8),                                         # 2^13: fused up to log_b = 7
             (0, 0), (0, 3), (0, 11), (3, 9)]                                # single-element and tiny columns; domains below 2^11 too


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("log_n,log_b", LDE_PAIRS)
def test_lde_and_evaluate_at_the_zero_extension_limit(kind, log_n, log_b, offset):
    """blow-ups below, at and beyond the first radix of a two-pass domain, subgroup and coset; two or three columns"""
    lde_and_evaluate(backends.planner(kind), log_n, log_b, offset, ncols=3 if log_n + log_b < 13 else 2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("log_n,log_b", [(13, 4), (11, 6), (17, 0)])
def test_lde_and_evaluate_three_passes(kind, log_n, log_b, op, monkeypatch):
    """A 2^17 domain in three passes, (6, 6, 5): the bit-reversed store of the last pass places the middle digit by brev(mid, log_r1) with
    log_r1 != 0, and the zero extension stops at lr0 = 6 -- blow-up 16 inside it, 64 at it, 1 without any.  (One call per case: a 2^17
    transform takes the simulator most of a second.)"""
    with fresh_planner(kind, monkeypatch, MS_NTT252_PASSES=3) as (pl, keep):
        lde_and_evaluate(pl, log_n, log_b, 3, ncols=2, passes=3, keep=keep, ops=(op,))


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,log_b", [(14, 4), (12, 6)])
def test_lde_and_evaluate_2_18_hip(log_n, log_b):
    """a 2^18 domain, (9, 9): tiles of 512 rows of which 32 or 8 hold coefficients"""
    lde_and_evaluate(backends.planner("hip"), log_n, log_b, 3, ncols=2)
