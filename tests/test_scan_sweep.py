"""Sweep of ms_scan_affine through the C ABI: every scan_reduce / scan_apply / scan_blocks instantiation csrc/ms_stage.cpp can launch, at the
lengths where the tile, the block walk and the choice of instantiation change.  Every output word is compared, bit-exact; every buffer
carries guard words behind its last element and every input is compared after the call.

The instantiations.  scan_rows_per_lane (ms_stage.cpp), restated below as rows_per_lane(): 4 rows per lane below 2^20 rows and for the
252-bit field at every length, from 2^20 rows on 16 for Fp and 8 for Fq3.  A workgroup has 256 lanes, so a block is T4 = 1024, T8 = 2048
or T16 = 4096 rows.  scan_blocks is one workgroup: lane t walks chunk = ceil(nblocks / 256) consecutive block aggregates.  The map kind
(a: multipliers only, b: addends only, ab: both) is a template argument of all three kernels.

    field   rows/lane  kinds     lengths below that reach it                                       chunk
    Fp          4      a b ab    1 .. 2T4+5 | 256 T4 | 256 T4 + 1 | 512 T4 + 1 | 2^20 - 1           1 | 1 | 2 | 3 | 4
    Fq3         4      a b ab    1 .. 2T4+5 | 256 T4 | 256 T4 + 1                                   1 | 1 | 2
    Fp252       4      a b ab    1 .. 2T4+5 | 256 T4 | 256 T4 + 1 | 2^20 (ab only)                  1 | 1 | 2 | 4
    Fp         16      a b ab    2^20 (256 blocks) | 2^20 + 1 | 2^20 + 3 T4 + 7                     1 | 2 | 2
    Fq3         8      a b ab    2^20 (512 blocks) | 2^20 + 1 (513 blocks) | 2^20 + 3 T4 + 7        2 | 3 | 3

That is 15 rows of scan_reduce / scan_apply (field x kind x rows per lane) and 9 of scan_blocks (field x kind); INSTANTIATIONS lists them
and test_every_instantiation_walks_blocks_in_chunks checks the cases below against it.  `inclusive` is a run-time flag: it alternates
along the long cases so that every row of the table sees both values at a multi-block length.

References (none shares code with the library).  Goldilocks: oracle.pyref.scan.scan_affine, the sequential loop on Python integers.  The loop
is run on the device's own words: the device keeps x as w(x) = x R mod p and its product is w(a) w(s) / R, so with the multipliers taken
out of Montgomery form (a = w(a) / R) and the addends and the state left as words, the loop `state = a * state + b` over the field IS the
recurrence of the words -- test_the_loop_on_words_is_the_loop_on_values pins that against the all-canonical route.  The 252-bit field: the
same loop on Python integers modulo F252.p, on the Montgomery words (tests/test_stage_sweep.py's M252).

One loop per (field, kind) over the longest length, inputs drawn once: a scan of the first n rows is a prefix of it, so every long case
slices the same sequence of states."""
import collections
import functools

import numpy as np
import pytest

from oracle.pyref import scan as oscan
from oracle.pyref import fields as PF
from tests import backends
from tests.test_stage_sweep import GL_EDGE, M252, Buf, same, gl_values
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as F252

P, P252 = PF.GL_P, PF.F252_P
V = {FP: 1, FQ3: 3, F252: 4}
FNAME = {FP: "fp", FQ3: "fq3", F252: "f252"}
FIELDS = (FP, FQ3, F252)
KINDS_OF_MAP = ("a", "b", "ab")
MS_OK, MS_ERR_INVALID = 0, -1
KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]

NT = 256                                   # lanes of a workgroup; also the lanes of scan_blocks' single workgroup
SWITCH = 1 << 20                           # from this many rows on, Fp and Fq3 leave 4 rows per lane
T4, T8, T16 = NT * 4, NT * 8, NT * 16      # rows of a block at 4, 8 and 16 rows per lane


def rows_per_lane(n, field):
    """scan_rows_per_lane's rule, restated"""
    return 4 if n < SWITCH or field == F252 else 16 if field == FP else 8


def blocks_and_chunk(n, field):
    nblocks = -(-n // (NT * rows_per_lane(n, field)))
    return nblocks, -(-nblocks // NT)


RAGGED = SWITCH + 3 * T4 + 7               # ends in row 7 of lane 192 of a T16 block, and in row 7 of lane 128 of a T8 block
SHORT = [1, 2, 3, 4, 5, T4 - 1, T4, T4 + 1, 2 * T4 + 5]
# (field, kind, rows per lane) -> the multi-block lengths of the sweep that reach it
INSTANTIATIONS = {}
for _f in FIELDS:
    for _k in KINDS_OF_MAP:
        INSTANTIATIONS[(_f, _k, 4)] = [NT * T4, NT * T4 + 1] + ([2 * NT * T4 + 1, SWITCH - 1] if _f == FP else []) + ([SWITCH] if (_f, _k) == (F252, "ab") else [])
for _k in KINDS_OF_MAP:
    INSTANTIATIONS[(FP, _k, 16)] = [SWITCH, SWITCH + 1, RAGGED]
    INSTANTIATIONS[(FQ3, _k, 8)] = [SWITCH, SWITCH + 1, RAGGED]
NMAX = {(f, k): max(n for (ff, kk, _), ns in INSTANTIATIONS.items() if (ff, kk) == (f, k) for n in ns) for f in FIELDS for k in KINDS_OF_MAP}


# ------------------------------------------------------------------------------------------------------------------
# values: Montgomery words as the device reads them
# ------------------------------------------------------------------------------------------------------------------
ONE = {FP: np.array([PF.GL_R], dtype=np.uint64), FQ3: np.array([PF.GL_R, 0, 0], dtype=np.uint64), F252: M252.words([M252.R])}


def draw(field, n, seed, nonzero=False):
    """n elements with the carry-edge words of tests/test_stage_sweep.py sprinkled in (GL_EDGE, the all-(p-1) Fq3 element, the Fp252 edge pool).
    nonzero: for multipliers -- a zero multiplier erases every state before it, and with it any wrong block carry -- zero elements become one."""
    v = V[field]
    a = (M252.values(n + 1, seed) if field == F252 else gl_values(n + 1, v, seed))[:n * v].reshape(n, v)      # their last element is zero: dropped
    if nonzero:
        a[~a.any(axis=1)] = ONE[field]
    return np.ascontiguousarray(a.reshape(-1))


def no_zero_element(a, field):
    return bool(np.asarray(a).reshape(-1, V[field]).any(axis=1).all())


def maps(field, n, seed):
    """(multipliers, addends): edge words, and masked rows (a = 1, b = 0: padding rows leave the state as it is) on one row in seven"""
    v = V[field]
    a, b = draw(field, n, seed, nonzero=True).reshape(n, v), draw(field, n, seed + 1).reshape(n, v)
    masked = np.random.default_rng(seed + 2).random(n) < 1 / 7
    a[masked] = ONE[field]
    b[masked] = 0
    return np.ascontiguousarray(a.reshape(-1)), np.ascontiguousarray(b.reshape(-1))


def inits(field):
    """0, 1, the word p - 1 (the largest canonical word, in every component) and the element -1, as Montgomery words"""
    v = V[field]
    if field == F252:
        return [np.zeros(4, dtype=np.uint64), ONE[F252].copy(), M252.words([P252 - 1]), M252.words([P252 - M252.R])]
    return [np.zeros(v, dtype=np.uint64), ONE[field].copy(), np.full(v, P - 1, dtype=np.uint64), np.array([P - PF.GL_R] + [0] * (v - 1), dtype=np.uint64)]


LONG_INIT = {"a": 2, "b": 0, "ab": 1}      # index into inits(): a running product from p - 1, a running sum from 0, a running evaluation from 1


# ------------------------------------------------------------------------------------------------------------------
# references: the sequence of states s_0 = init, s_1, ..., s_n as words, [n + 1, V]
# ------------------------------------------------------------------------------------------------------------------
def _elems(words, v):
    xs = [int(w) for w in words]
    return xs if v == 1 else [tuple(xs[i:i + 3]) for i in range(0, len(xs), 3)]


def _out_of_mont(words, v):
    xs = ((np.asarray(words).astype(object) * PF.GL_RINV) % P).tolist()
    return xs if v == 1 else [tuple(xs[i:i + 3]) for i in range(0, len(xs), 3)]


def states(field, a, b, init, n):
    v = V[field]
    if field == F252:
        A, B = (M252.ints(a) if a is not None else None), (M252.ints(b) if b is not None else None)
        s = M252.ints(init)[0]
        seq = [s]
        for i in range(n):
            if A is not None:
                s = M252.mul(A[i], s)
            if B is not None:
                s = M252.add(s, B[i])
            seq.append(s)
        return M252.words(seq).reshape(n + 1, 4)
    first = _elems(init, v)[0]
    after = oscan.scan_affine(_out_of_mont(a, v) if a is not None else None, _elems(b, v) if b is not None else None, first, n, v == 3, True)
    return np.array([first] + after, dtype=np.uint64).reshape(n + 1, v)


def expected(seq, n, inclusive):
    return np.ascontiguousarray(seq[1:n + 1] if inclusive else seq[:n]).reshape(-1)


@functools.lru_cache(maxsize=None)
def long_inputs(field):
    n = max(NMAX[(field, k)] for k in KINDS_OF_MAP)
    return maps(field, n, 4000 + field)


@functools.lru_cache(maxsize=None)
def long_states(field, kind):
    """one loop per (field, kind), over the longest length the table lists for it; every long case is a prefix"""
    n = NMAX[(field, kind)]
    a, b = long_inputs(field)
    v = V[field]
    return states(field, a[:n * v] if "a" in kind else None, b[:n * v] if "b" in kind else None, inits(field)[LONG_INIT[kind]], n)


def test_the_loop_on_words_is_the_loop_on_values():
    """oracle.pyref.scan on canonical values, its result put into Montgomery form, against the route of `states` (multipliers canonical, addends
    and state as words); and the 252-bit loop against plain arithmetic on canonical integers"""
    n = 300
    for field, F in ((FP, PF.GL), (FQ3, PF.FQ3)):
        v = V[field]
        a, b = maps(field, n, 5)
        init = inits(field)[3]
        ca, cb, c0 = _out_of_mont(a, v), _out_of_mont(b, v), _out_of_mont(init, v)[0]
        want = [c0] + oscan.scan_affine(ca, cb, c0, n, v == 3, True)
        flat = want if v == 1 else [c for t in want for c in t]
        assert np.array_equal(states(field, a, b, init, n).reshape(-1), np.array([PF.GL.to_mont(x) for x in flat], dtype=np.uint64))
    a, b = maps(F252, n, 6)
    init = inits(F252)[3]
    G = PF.F252
    s = G.from_mont(M252.ints(init)[0])
    assert s == P252 - 1
    want = [s]
    for x, y in zip(M252.ints(a), M252.ints(b)):
        s = (G.from_mont(x) * s + G.from_mont(y)) % P252
        want.append(s)
    assert M252.ints(states(F252, a, b, init, n)) == [G.to_mont(x) for x in want]


# ------------------------------------------------------------------------------------------------------------------
# one call
# ------------------------------------------------------------------------------------------------------------------
def run_scan(pl, field, kind, n, inclusive, a, b, init, want, what):
    """a, b: the words of n elements (used or not by the kind); want: the expected words"""
    L, v = pl.lib, V[field]
    A = Buf(pl, a) if "a" in kind else None
    B = Buf(pl, b) if "b" in kind else None
    if A is not None:
        assert no_zero_element(a, field), "a zero multiplier would hide a wrong carry: the case is void"
    D = Buf.junk(pl, n * v)
    rc = L.ms_scan_affine(pl.handle, field, n, A.ptr if A else None, B.ptr if B else None, init.ctypes.data, int(inclusive), D.ptr)
    assert rc == MS_OK, L.ms_last_error()
    same(D.read(), want, what)
    if A is not None:
        same(A.read(), a, what + ": the multipliers")
    if B is not None:
        same(B.read(), b, what + ": the addends")


# ------------------------------------------------------------------------------------------------------------------
# short lengths: one block and its edges, the three kinds, inclusive and exclusive, each with the four inits
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inclusive", [False, True], ids=["exclusive", "inclusive"])
@pytest.mark.parametrize("mapkind", KINDS_OF_MAP)
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
def test_short_lengths(kind, field, mapkind, inclusive):
    pl, v = backends.planner(kind), V[field]
    a, b = maps(field, SHORT[-1], 100 + field)
    for n in SHORT:
        for init in inits(field):
            seq = states(field, a[:n * v] if "a" in mapkind else None, b[:n * v] if "b" in mapkind else None, init, n)
            run_scan(pl, field, mapkind, n, inclusive, a[:n * v], b[:n * v], init, expected(seq, n, inclusive), f"n = {n}, init {init.tolist()}")


# ------------------------------------------------------------------------------------------------------------------
# the block walk and the switch of instantiation
# ------------------------------------------------------------------------------------------------------------------
Walk = collections.namedtuple("Walk", "field mapkind n inclusive per kinds")


def _walks():
    """every (instantiation, length) of INSTANTIATIONS; `inclusive` alternates along the lengths of an instantiation (shifted by the kind).
    The simulator runs one length with chunk >= 2 per instantiation (256 T4 + 1 at 4 rows per lane); the device runs them all."""
    out = []
    for (field, mapkind, per), lengths in INSTANTIATIONS.items():
        ki = KINDS_OF_MAP.index(mapkind)
        for li, n in enumerate(lengths):
            assert rows_per_lane(n, field) == per
            if n < SWITCH:
                emu = n == NT * T4 + 1
            elif field == F252:
                emu = False                                         # 4 rows per lane with chunk 2 runs on the simulator at 256 T4 + 1
            else:
                emu = n == (SWITCH + 1, RAGGED, SWITCH + 1)[ki]
            out.append(Walk(field, mapkind, n, bool((li + ki) % 2), per, ("emu", "hip") if emu else ("hip",)))
    return out


WALKS = _walks()


def walk_id(w):
    return f"{FNAME[w.field]}-{w.mapkind}-per{w.per}-n{w.n}-{'inclusive' if w.inclusive else 'exclusive'}"


@pytest.mark.parametrize("kind,walk", [pytest.param(kind, w, id=kind + "-" + walk_id(w), marks=[pytest.mark.gpu] if kind == "hip" else [])
                                       for w in WALKS for kind in w.kinds])
def test_block_walk(kind, walk):
    field, mapkind, n, v = walk.field, walk.mapkind, walk.n, V[walk.field]
    a, b = long_inputs(field)
    run_scan(backends.planner(kind), field, mapkind, n, walk.inclusive, a[:n * v], b[:n * v], inits(field)[LONG_INIT[mapkind]],
             expected(long_states(field, mapkind), n, walk.inclusive), walk_id(walk))


def test_every_instantiation_walks_blocks_in_chunks():
    """the table of the docstring, checked: 15 reduce / apply instantiations, each with a case of chunk >= 2 on both backends and both values of
    `inclusive` at a multi-block length on the device; the block counts at the edges are the ones the table names"""
    assert len(INSTANTIATIONS) == 15
    assert {(f, k) for f, k, _ in INSTANTIATIONS} == {(f, k) for f in FIELDS for k in KINDS_OF_MAP}
    assert {per for f, k, per in INSTANTIATIONS if f == FP} == {4, 16} and {per for f, k, per in INSTANTIATIONS if f == FQ3} == {4, 8}
    assert {per for f, k, per in INSTANTIATIONS if f == F252} == {4}
    for (field, mapkind, per), lengths in INSTANTIATIONS.items():
        mine = [w for w in WALKS if (w.field, w.mapkind, w.per) == (field, mapkind, per)]
        assert [w.n for w in mine] == lengths
        for backend in ("emu", "hip"):
            assert any(blocks_and_chunk(w.n, field)[1] >= 2 for w in mine if backend in w.kinds), (FNAME[field], mapkind, per, backend)
        assert {w.inclusive for w in mine if "hip" in w.kinds and blocks_and_chunk(w.n, field)[0] > 1} == {False, True}
    assert blocks_and_chunk(NT * T4, FP) == (256, 1) and blocks_and_chunk(NT * T4 + 1, F252) == (257, 2)
    assert blocks_and_chunk(2 * NT * T4 + 1, FP) == (513, 3) and blocks_and_chunk(SWITCH - 1, FP) == (1024, 4)
    assert blocks_and_chunk(SWITCH, FP) == (256, 1) and blocks_and_chunk(SWITCH, FQ3) == (512, 2) and blocks_and_chunk(SWITCH, F252) == (1024, 4)
    assert blocks_and_chunk(SWITCH + 1, FP) == (257, 2) and blocks_and_chunk(SWITCH + 1, FQ3) == (513, 3)
    assert (RAGGED % T16) % 16 == 7 and (RAGGED % T8) % 8 == 7 and RAGGED % T4 == 7
    for field in FIELDS:
        a, _ = long_inputs(field)
        assert no_zero_element(a, field)
        assert any(np.array_equal(a.reshape(-1, V[field])[i], ONE[field]) for i in range(64))          # masked rows are there
    assert np.isin(GL_EDGE[1:], long_inputs(FP)[0]).all() and (long_inputs(FQ3)[0].reshape(-1, 3) == np.uint64(P - 1)).all(axis=1).any()


# ------------------------------------------------------------------------------------------------------------------
# a = 0 itself: one zero multiplier at a known row of the second block, the whole column checked
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
def test_one_zero_multiplier_in_the_second_block(kind, field):
    pl, v, n, row = backends.planner(kind), V[field], 2 * T4 + 5, T4 + 77
    a, b = maps(field, n, 300 + field)
    a[row * v:(row + 1) * v] = 0
    assert int((~a.reshape(n, v).any(axis=1)).sum()) == 1
    init = inits(field)[2]
    L = pl.lib
    for mapkind in ("a", "ab"):
        seq = states(field, a, b if "b" in mapkind else None, init, n)
        if mapkind == "a":
            assert seq[row].any() and not seq[row + 1:].any()          # the product dies after that row, not before
        for inclusive in (False, True):
            A, B, D = Buf(pl, a), Buf(pl, b), Buf.junk(pl, n * v)
            assert L.ms_scan_affine(pl.handle, field, n, A.ptr, B.ptr if "b" in mapkind else None, init.ctypes.data, int(inclusive), D.ptr) == MS_OK
            same(D.read(), expected(seq, n, inclusive), f"{mapkind}, inclusive {inclusive}")
            same(A.read(), a, "the multipliers")


# ------------------------------------------------------------------------------------------------------------------
# in place: d_out == d_a, d_out == d_b, d_a == d_b == d_out -- at a multi-block length of every rows-per-lane value
# ------------------------------------------------------------------------------------------------------------------
IN_PLACE = {4: (F252, 3 * T4 + 5), 8: (FQ3, SWITCH + 1), 16: (FP, SWITCH + 1)}


@functools.lru_cache(maxsize=None)
def squared_states(field, n):
    """d_a == d_b: state = a * state + a"""
    a = long_inputs(field)[0][:n * V[field]]
    return states(field, a, a, inits(field)[1], n)


# the simulator runs a 2^20-row Fq3 scan in seconds: of the 8-rows-per-lane shapes it takes d_out == d_a only; the device takes all nine
@pytest.mark.parametrize("kind,per,which", [pytest.param(kind, per, which, id=f"{kind}-per{per}-{which}", marks=[pytest.mark.gpu] if kind == "hip" else [])
                                            for per in (4, 8, 16) for which in ("out_is_a", "out_is_b", "out_is_a_is_b") for kind in ("emu", "hip")
                                            if kind == "hip" or per != 8 or which == "out_is_a"])
def test_in_place(kind, per, which):
    pl = backends.planner(kind)
    L = pl.lib
    field, n = IN_PLACE[per]
    v = V[field]
    assert rows_per_lane(n, field) == per and blocks_and_chunk(n, field)[0] > 1
    a, b = (x[:n * v] for x in long_inputs(field))
    assert no_zero_element(a, field)
    init = inits(field)[1]
    inclusive = per != 8
    A, B = Buf(pl, a), Buf(pl, b)
    if which == "out_is_a_is_b":
        want = expected(squared_states(field, n), n, inclusive)
        assert L.ms_scan_affine(pl.handle, field, n, A.ptr, A.ptr, init.ctypes.data, int(inclusive), A.ptr) == MS_OK, L.ms_last_error()
        same(A.read(), want, which)
        return
    want = expected(long_states(field, "ab"), n, inclusive)                     # LONG_INIT["ab"] is init 1 as well
    out, other, words = (A, B, b) if which == "out_is_a" else (B, A, a)
    assert L.ms_scan_affine(pl.handle, field, n, A.ptr, B.ptr, init.ctypes.data, int(inclusive), out.ptr) == MS_OK, L.ms_last_error()
    same(out.read(), want, which)
    same(other.read(), words, which + ": the other input")


# ------------------------------------------------------------------------------------------------------------------
# partial overlaps of d_out with an input are refused before anything is enqueued; d_a over d_b is not
# ------------------------------------------------------------------------------------------------------------------
N_AL = 300


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["out_one_element_into_a", "out_one_element_into_b", "out_one_element_before_a"])
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
def test_partial_overlap_is_refused(kind, field, shape):
    pl, v, n = backends.planner(kind), V[field], N_AL
    L = pl.lib
    a, b = maps(field, n + 1, 700 + field)                  # the arena: one spare element | a (n + 1 elements) | b (n + 1) | free space
    before = np.concatenate([ONE[field], a, b, np.full((n + 1) * v, 0xDEADBEEFDEADBEEF, dtype=np.uint64)])
    arena = Buf(pl, before)
    esz = 8 * v
    pa, pb = arena.ptr + esz, arena.ptr + esz * (n + 2)
    out = {"out_one_element_into_a": pa + esz, "out_one_element_into_b": pb + esz, "out_one_element_before_a": pa - esz}[shape]
    init = inits(field)[1]
    rc = L.ms_scan_affine(pl.handle, field, n, pa, pb, init.ctypes.data, 0, out)
    msg = L.ms_last_error()
    assert rc == MS_ERR_INVALID, f"{shape}: returned {rc}"          # stop here: the words of an accepted call are never looked at
    assert b"overlap" in msg and b"ms_scan_affine" in msg and (b"d_b" if shape.endswith("_b") else b"d_a") in msg, msg
    pl.sync()
    same(arena.read(), before, "the arena after a refused call")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
def test_overlapping_inputs_and_touching_buffers_are_allowed(kind, field):
    """d_a and d_b are only read: d_b one element into d_a, and d_b == d_a, give the loop's words; so does an output that starts where an input ends"""
    pl, v, n = backends.planner(kind), V[field], 2 * T4 + 5
    L = pl.lib
    x = draw(field, n + 1, 800 + field, nonzero=True)
    init = inits(field)[3]
    for shift in (1, 0):
        X, D = Buf(pl, x), Buf.junk(pl, n * v)
        a, b = x[:n * v], x[shift * v:(n + shift) * v]
        assert L.ms_scan_affine(pl.handle, field, n, X.ptr, X.ptr + 8 * v * shift, init.ctypes.data, 1, D.ptr) == MS_OK, L.ms_last_error()
        same(D.read(), expected(states(field, a, b, init, n), n, True), f"d_b = d_a + {shift} elements")
        same(X.read(), x, "the inputs")
    a, b = maps(field, n, 810 + field)
    junk = np.full(n * v, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    X = Buf(pl, np.concatenate([a, junk, b]))                              # a | out | b, each starting where the one before ends
    assert L.ms_scan_affine(pl.handle, field, n, X.ptr, X.ptr + 16 * n * v, init.ctypes.data, 0, X.ptr + 8 * n * v) == MS_OK, L.ms_last_error()
    same(X.read(), np.concatenate([a, expected(states(field, a, b, init, n), n, False), b]), "adjacent buffers")
