"""Sweep of the DEEP entry points through the C ABI (ms_horner_eval, ms_deep_compose, ms_deep_rows), with the ctypes argument lists built
here, so that points, terms, `first` and `count` are free: DeepPolyComposer can only produce the prover's shapes.  Every test runs on the
simulator build and, marked gpu, on the device.  Every output word is compared, bit-exact; every output buffer carries guard words behind
its last element; every input column is compared after the call.  References: tests/deep_ref.py (none shares code with csrc/).

Kernel instantiations that csrc/ms_deep.cpp can launch, and the test that reaches each (test_the_table_names_every_launch compares
this table with the hipLaunchKernelGGL lines of ms_deep.cpp and with the cases below):

  instantiation                               reached when                                   test
  ------------------------------------------  ---------------------------------------------  ------------------------------------
  msdeep::horner_blocks<1,1,2>  (level 0)     Fp coefficients, Fp points                     test_horner[*-fpxfp-*]
  msdeep::horner_blocks<1,3,2>  (level 0)     Fp coefficients, Fq3 points                    test_horner[*-fpxfq3-*]
  msdeep::horner_blocks<3,3,2>  (level 0)     Fq3 coefficients, Fq3 points                   test_horner[*-fq3xfq3-*]
  msdeep::horner_blocks<3,3,2>  (level >= 1)  n > 4096 (two levels), n > 4096^2 (three)      test_horner[*-n2048[0-9]*], test_horner_three_levels
  msdeep252::horner_blocks                    the 252-bit field                              test_horner[*-f252xf252-*]
  compose: msdeep::deep_points<1,4,3>         Fp, npoints <= 3, n >= 4096                    test_compose[*-fp-log1[23]-np3-*]
  compose: msdeep::deep_points<1,1,8>         Fp otherwise                                   test_compose[*-fp-*-np5-*], log_n < 12
  compose: msdeep::deep_points<3,2,4>         Fq3, npoints <= 4, n >= 4096                   test_compose[*-fq3-log1[23]-np4-*]
  compose: msdeep::deep_points<3,1,8>         Fq3 otherwise                                  test_compose[*-fq3-*-np6-*], log_n < 12
  rows:    msdeep::deep_points<1,2,3>         Fp, npoints <= 3, count >= 4096                test_rows[*-fp-*] with count >= 4096, np <= 3
  rows:    msdeep::deep_points<1,1,8>         Fp otherwise                                   test_rows[*-fp-*]
  rows:    msdeep::deep_points<3,2,4>         Fq3, npoints <= 4, count >= 4096               test_rows[*-fq3-*] with count >= 4096, np <= 4
  rows:    msdeep::deep_points<3,1,8>         Fq3 otherwise                                  test_rows[*-fq3-*]
  msdeep::deep_degree_adjust<1>               every Fp compose                               test_compose[*-fp-*]
  msdeep::deep_degree_adjust<3>               every Fq3 compose                              test_compose[*-fq3-*]
  msdeep252::deep_points                      252-bit compose                                test_compose[*-f252-*]
  msdeep252::deep_degree_adjust               252-bit compose                                test_compose[*-f252-*]
  msdeep252::deep_rows<4,4>                   252-bit rows                                   test_rows[*-f252-*]

Sizes trimmed under the simulator (kinds of case are not): ms_horner_eval at n around 4096^2 runs one of its three lengths there
(4096^2 + 1, the three-level one); the 252-bit domain of 2^22 points (the smallest whose two-level twiddle table has an upper level:
lo_bits = min(21, log_n) in ms_ntt_plan.cpp) runs on the device only.

Rules pinned here and stated in include/ministark_hip.h: log_n = 0 and 1 of ms_deep_compose give the reference's words; nterms = 0 gives
an all-zero output; d_out overlapping an input column is refused (MS_ERR_INVALID, "overlap") before anything is enqueued."""
import collections
import os
import re

import numpy as np
import pytest

from tests import backends
from tests.deep_ref import *          # noqa: F401,F403  (the helpers' names are listed in its __all__)

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FNAME = {FP: "fp", FQ3: "fq3", F252: "f252"}
FIELDS = (FP, FQ3, F252)
# terms per point, by number of points: every count of {0, 1, 15, 16, 17, 31, 32, 33, 48} appears, mixed within a call
LAYOUT = {1: [48], 2: [17, 16], 3: [33, 0, 15], 4: [16, 32, 1, 31], 5: [31, 0, 17, 15, 1], 6: [1, 16, 0, 33, 15, 17],
          7: [15, 1, 32, 0, 16, 17, 31], 8: [0, 1, 15, 16, 17, 31, 32, 48]}
assert {c for v in LAYOUT.values() for c in v} == {0, 1, 15, 16, 17, 31, 32, 33, 48}
COUNTS = [1, 63, 64, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 4096 + 511, 3 * 4096 + 17]
COUNTS252 = [1023, 1024, 1025, 2049]                  # a workgroup of msdeep252::deep_rows<4,4> takes 1024 rows
POINT_KINDS = [(), ("base",), ("zero",), ("x",), ("rand", "zero", "x", "base")]
OFFSETS = [None, 1, "other"]
DEGREES = ["rand", "b0", "a0", "one"]
LOG_MAIN = 14                                          # 2^14 >= 3 * 4096 + 17; Goldilocks lo_bits = min(12, log_n): the upper table level is in use


def point_kinds(field, kinds):
    return kinds if field == FQ3 else tuple(k if k == "zero" else "rand" for k in kinds)


def columns_of(field, n, special, seed, density=0.3):
    """-> base words, ext words, the column no term names.  Default: five base columns (mixed, unnamed, all p - 1, all zero, mixed or -- 252-bit --
    all 2^251 - 1) and, over Fq3, three extension columns."""
    if special == "cols96":
        return ([column(FP if field != F252 else F252, n, "mix", seed + c, density) for c in range(96)],
                [column(FQ3, n, "mix", seed + 100 + c, density) for c in range(96)] if field == FQ3 else [], None)
    kinds = ["mix", "mix", "pm1", "zero", "top" if field == F252 else "mix"]
    base = [column(F252 if field == F252 else FP, n, k, seed + c, density) for c, k in enumerate(kinds)]
    ext = [column(FQ3, n, "mix", seed + 10 + c, density) for c in range(3)] if field == FQ3 else []
    if special == "nbase0":
        return [], ext, None
    if special == "next0":
        return base, [], 1
    return base, ext, 1


# ------------------------------------------------------------------------------------------------------------------
# ms_deep_rows
# ------------------------------------------------------------------------------------------------------------------
Rows = collections.namedtuple("Rows", "field ld first count np offset degree pkinds special kinds")


def rows_shape(field, npoints, count):
    """the dispatch of ms_deep_rows, restated by hand"""
    if field == F252:
        return "msdeep252::deep_rows<4,4>"
    if field == FP:
        return "msdeep::deep_points<1,2,3>" if npoints <= 3 and count >= 4096 else "msdeep::deep_points<1,1,8>"
    return "msdeep::deep_points<3,2,4>" if npoints <= 4 and count >= 4096 else "msdeep::deep_points<3,1,8>"


def _rows_cases():
    out = []
    both = ("emu", "hip")
    for fi, f in enumerate(FIELDS):
        N = 1 << LOG_MAIN
        for ci, count in enumerate(COUNTS + (COUNTS252 if f == F252 else [])):
            i = ci + fi
            first = [0, 1, 777, N - count][i % 4]
            out.append(Rows(f, LOG_MAIN, min(first, N - count), count, 1 + i % 8, OFFSETS[i % 3], DEGREES[i % 4], POINT_KINDS[i % 5], None, both))
        # both sides of the launch threshold (3 | 4 points over Fp, 4 | 5 over Fq3) and the widest call, at ragged counts of 4096 and more
        lo = 3 if f != FQ3 else 4
        for j, (np_, count) in enumerate(((lo, 4097), (lo + 1, 4097), (8, 4096 + 511), (lo, 3 * 4096 + 17), (lo + 1, 4096), (lo, 4096), (1, 4096 + 511),
                                          (lo + 1, 3 * 4096 + 17))):
            first = [1, N - count, 777, 0][j % 4]
            out.append(Rows(f, LOG_MAIN, min(first, N - count), count, np_, OFFSETS[j % 3], DEGREES[(j + 1) % 4], POINT_KINDS[(j + 2) % 5], None, both))
        # xshift = max(log_domain, 12) - log_domain; the whole domain and all of it but row 0
        for j, ld in enumerate((1, 2, 11, 12, 13)):
            N2 = 1 << ld
            out.append(Rows(f, ld, 0, N2, 1 + (j + fi) % 8, OFFSETS[j % 3], DEGREES[j % 4], POINT_KINDS[j % 5], None, both))
            out.append(Rows(f, ld, 1, N2 - 1, 8 - (j + fi) % 8, OFFSETS[(j + 1) % 3], DEGREES[(j + 2) % 4], POINT_KINDS[(j + 3) % 5], None, both))
        out.append(Rows(f, 12, 5, 300, 3, None, "rand", (), "nterms0", both))
        out.append(Rows(f, 12, 5, 257, 2, None, "rand", (), "cols96", both))
        out.append(Rows(f, 13, 777, 4097, 3 if f != FQ3 else 4, None, "rand", ("zero",), "heavy", both))      # see test_the_reduction_edges_are_reached
        if f == FQ3:
            out.append(Rows(f, 12, 3, 300, 5, 1, "rand", ("base", "x"), "nbase0", both))
            out.append(Rows(f, 13, 3, 4099, 4, None, "rand", ("base", "x"), "next0", both))
        if f == F252:
            # lo_bits = min(21, log_n) for the 252-bit tables (ms_ntt_plan.cpp): 2^22 points is the smallest domain with an upper level, and
            # bitrev(first + i) >= 2^21 at every odd position
            out.append(Rows(f, 22, (1 << 21) + 12345, 1025, 3, None, "rand", (), None, ("hip",)))
    return out


def rows_id(c):
    return (f"{FNAME[c.field]}-ld{c.ld}-first{c.first}-count{c.count}-np{c.np}-off{c.offset}-{c.degree}" + ("-" + "_".join(c.pkinds) if c.pkinds else "")
            + ("-" + c.special if c.special else ""))


ROWS = _rows_cases()


def rows_inputs(c, seed, density=0.3):
    f = c.field
    N = 1 << c.ld
    h, _ = offset_of(f, c.offset)
    base, ext, skip = columns_of(f, c.count, c.special, seed, density)
    counts = [0] * c.np if c.special == "nterms0" else ([2, 1] if c.special == "cols96" else LAYOUT[c.np])
    heavy = None
    if c.special == "heavy":      # point 0: every term on the all-(p - 1) column (252-bit: the all-(2^251 - 1) column) with the largest alpha
        heavy = (0, 4, M252.words([TOP252])) if f == F252 else (0, 2, np.full(PW[f], P - 1, dtype=np.uint64))
    if c.special == "cols96":
        ncols = len(base) + len(ext)
        tcol, tpoint = list(range(ncols)), [k % 2 for k in range(ncols)]
        alpha, ood = words(f, ncols, seed + 50, density), words(f, ncols, seed + 51, density)
    else:
        tcol, tpoint, alpha, ood = terms_of(f, counts, len(base) + len(ext), skip, seed + 50, density, heavy)
    points = points_of(f, c.np, point_kinds(f, c.pkinds), h, N, seed + 60)
    da, db = degree_of(f, c.degree, seed + 70)
    return base, ext, points, tcol, tpoint, alpha, ood, da, db


def run_rows(pl, c, seed):
    base, ext, points, tcol, tpoint, alpha, ood, da, db = rows_inputs(c, seed)
    got = check_rows(pl, c.field, c.ld, c.first, c.count, c.offset, base, ext, points, tcol, tpoint, alpha, ood, da, db, seed, rows_id(c))
    if c.special == "nterms0":
        assert not got.any(), "no terms: the output is all zero"


@pytest.mark.parametrize("kind,case", [pytest.param(k, c, id=k + "-" + rows_id(c), marks=[pytest.mark.gpu] if k == "hip" else []) for c in ROWS for k in c.kinds])
def test_rows(kind, case):
    run_rows(backends.planner(kind), case, 3000 + 11 * ROWS.index(case))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
def test_rows_do_not_depend_on_the_split(kind, field):
    """one ragged domain cut at unaligned places, a one-row shard among them: the shards' words are the whole call's words.  The whole call
    and the long shard take the count >= 4096 launch, the short ones the generic one; the pooled inversions group other rows every time."""
    pl = backends.planner(kind)
    ld, np_ = 13, (3 if field != FQ3 else 4)
    N, pw = 1 << ld, PW[field]
    c = Rows(field, ld, 0, N, np_, None, "rand", ("zero",), None, None)
    base, ext, points, tcol, tpoint, alpha, ood, da, db = rows_inputs(c, 4242)
    whole = check_rows(pl, field, ld, 0, N, None, base, ext, points, tcol, tpoint, alpha, ood, da, db, 1, "the whole domain")
    cuts = [0, 1, 778, 779, 1805, 2829, 2830, N - 4097, N]
    assert any(b - a >= 4096 for a, b in zip(cuts, cuts[1:])) and any(b - a == 1 for a, b in zip(cuts, cuts[1:]))
    for a, b in zip(cuts, cuts[1:]):
        cb, ce = [Buf(pl, w[a * (pw if field == F252 else 1):b * (pw if field == F252 else 1)]) for w in base], [Buf(pl, w[3 * a:3 * b]) for w in ext]
        out = Buf.junk(pl, (b - a) * pw)
        assert call_deep(pl, "rows", field, (ld, None, a, b - a), cb, ce, points, tcol, tpoint, alpha, ood, da, db, out.ptr) == MS_OK
        pl.sync()
        same(out.read(), whole[a * pw:b * pw], f"rows [{a}, {b})")


def _s5_and_sum(vs, alphas):
    """the exact sum of products of one window and component, and the sixth limb column: sum of (v >> 32) (alpha >> 44)"""
    return sum(v * a for v, a in zip(vs, alphas)), sum((v >> 32) * (a >> 44) for v, a in zip(vs, alphas))


def test_the_reduction_edges_are_reached():
    """CPU only, exact Python integers: what the inputs of the sweep's cases put into the accumulators.

    Goldilocks (limb_mac / limb_sum_reduce / reduce_132): over the (row, point, window of sixteen terms, component) sums of products
    column word x alpha word of base columns, at least one has the high word of the 128-bit sum >= p, one has the exact sum >= 2^128, and
    one has S[5] >> 52 non-zero (S[5] = sum of (v >> 32) (alpha >> 44)).  Uniform words reach none of them.

    252-bit (f252::mac81): the largest of the nineteen digit columns that sixteen canonical terms can produce is
    16 * 8 (2^28 - 1)^2 = 9223371968135299200 < 2^63: column 7, eight products of full 28-bit digits, both operands 2^251 - 1 (column 8 has
    nine products, but two of them carry the ninth digit, below 2^27; an operand of 2^251 or more, at most p - 1, has a ninth digit of 2^27
    and almost nothing below it, and gives less).  The `heavy` case fills a window with exactly those operands and reaches
    9223371968135299200, the same value: within the factor of 2 asked for, with nothing to spare."""
    seen = {"hi>=p": 0, "sum>=2^128": 0, "S5>>52": 0}
    for c in ROWS:
        if c.field == F252 or c.count > 600 and c.special != "heavy":
            continue
        base, ext, points, tcol, tpoint, alpha, ood, da, db = rows_inputs(c, 3000 + 11 * ROWS.index(c))
        pw = PW[c.field]
        for k in range(c.np):
            mine = [t for t in range(len(tcol)) if tpoint[t] == k]
            for t0 in range(0, len(mine), 16):
                win = [t for t in mine[t0:t0 + 16] if tcol[t] < len(base)]
                for row in range(0, min(c.count, 64)):
                    for w in range(pw):
                        tot, s5 = _s5_and_sum([int(base[tcol[t]][row]) for t in win], [int(alpha[t * pw + w]) for t in win])
                        seen["hi>=p"] += ((tot >> 64) & ((1 << 64) - 1)) >= P
                        seen["sum>=2^128"] += tot >= (1 << 128)
                        seen["S5>>52"] += (s5 >> 52) != 0
    assert all(seen.values()), seen
    # mac81
    M = (1 << 28) - 1
    digits = lambda x: [(x >> (28 * i)) & M for i in range(9)]
    col_max = lambda x, y: max(sum(digits(x)[i] * digits(y)[k - i] for i in range(9) if 0 <= k - i < 9) for k in range(17))
    possible = 16 * max(col_max(TOP252, TOP252), col_max(P252 - 1, TOP252), col_max(P252 - 1, P252 - 1))
    assert possible == 16 * 8 * M * M == 9223371968135299200 < (1 << 63)
    c = next(c for c in ROWS if c.field == F252 and c.special == "heavy")
    base, ext, points, tcol, tpoint, alpha, ood, da, db = rows_inputs(c, 3000 + 11 * ROWS.index(c))
    cols, al = [M252.ints(b[:4 * 8]) for b in base], M252.ints(alpha)
    reached = 0
    for k in range(c.np):
        mine = [t for t in range(len(tcol)) if tpoint[t] == k]
        for t0 in range(0, len(mine), 16):
            for row in range(8):
                sums = [0] * 17
                for t in mine[t0:t0 + 16]:
                    x, y = digits(cols[tcol[t]][row]), digits(al[t])
                    for kk in range(17):
                        sums[kk] += sum(x[i] * y[kk - i] for i in range(9) if 0 <= kk - i < 9)
                reached = max(reached, max(sums))
    assert 2 * reached >= possible and reached <= possible, (reached, possible)
    assert reached == 9223371968135299200


# ------------------------------------------------------------------------------------------------------------------
# ms_deep_compose
# ------------------------------------------------------------------------------------------------------------------
Compose = collections.namedtuple("Compose", "field log_n np offset degree pkinds special")


def compose_shape(field, npoints, n):
    if field == F252:
        return "msdeep252::deep_points"
    if field == FP:
        return "msdeep::deep_points<1,4,3>" if npoints <= 3 and n >= 4096 else "msdeep::deep_points<1,1,8>"
    return "msdeep::deep_points<3,2,4>" if npoints <= 4 and n >= 4096 else "msdeep::deep_points<3,1,8>"


def _compose_cases():
    out = []
    for fi, f in enumerate(FIELDS):
        lo = 3 if f != FQ3 else 4
        for j, log_n in enumerate((2, 8, 11, 12, 13)):
            for s, np_ in enumerate((lo, lo + 2)):
                i = j + s + fi
                out.append(Compose(f, log_n, np_, OFFSETS[i % 3], DEGREES[i % 4], POINT_KINDS[(i + 2 * s) % 5], None))
        for j, np_ in enumerate((1, 2, lo + 1, 7, 8)):                       # the rest of the term and point sweep
            out.append(Compose(f, 8, np_, OFFSETS[j % 3], DEGREES[(j + 1) % 4], POINT_KINDS[j % 5], None))
        out.append(Compose(f, 8, 3, None, "rand", (), "nterms0"))
        out.append(Compose(f, 6, 2, None, "rand", (), "cols96"))
        for log_n in (0, 1):                                                 # the reference's words: pinned here, stated in the header
            out.append(Compose(f, log_n, 2, None, "rand", ("zero",), None))
        if f == FQ3:
            out.append(Compose(f, 8, 5, 1, "rand", ("base", "x"), "nbase0"))
            out.append(Compose(f, 12, 4, None, "rand", ("base", "x"), "next0"))
    return out


def compose_id(c):
    return (f"{FNAME[c.field]}-log{c.log_n}-np{c.np}-off{c.offset}-{c.degree}" + ("-" + "_".join(c.pkinds) if c.pkinds else "") + ("-" + c.special if c.special else ""))


COMPOSE = _compose_cases()


def run_compose(pl, c, seed, density=0.3):
    f, pw, n = c.field, PW[c.field], 1 << c.log_n
    h, off = offset_of(f, c.offset)
    base, ext, skip = columns_of(f, n, c.special, seed, density)
    ncols = len(base) + len(ext)
    if c.special == "cols96":
        tcol, tpoint = list(range(ncols)), [k % 2 for k in range(ncols)]
        alpha = words(f, ncols, seed + 50, density)
    else:
        tcol, tpoint, alpha, _ = terms_of(f, [0] * c.np if c.special == "nterms0" else LAYOUT[c.np], ncols, skip, seed + 50, density)
    points = points_of(f, c.np, point_kinds(f, c.pkinds), h, n, seed + 60)
    if f == F252:
        assert not any(on_coset(f, points[4 * k:4 * k + 4], 5, n) for k in range(c.np))     # check_compose_252_identity evaluates on 5<w_n>
    da, db = degree_of(f, c.degree, seed + 70)
    ood = oods_252(base, points, tcol, tpoint) if f == F252 else oods_gl(f, base, ext, points, tcol, tpoint)
    B, E, out = [Buf(pl, w) for w in base], [Buf(pl, w) for w in ext], Buf.junk(pl, n * pw)
    rc = call_deep(pl, "compose", f, (c.log_n, off), B, E, points, tcol, tpoint, alpha, ood, da, db, out.ptr)
    assert rc == MS_OK, pl.lib.ms_last_error().decode()
    pl.sync()
    got = out.read()
    if f != F252:
        same(got, ref_compose_gl(f, n, base, ext, points, tcol, tpoint, alpha, da, db), compose_id(c))
    elif c.log_n <= 8:
        same(got, ref_compose_252_division(n, base, points, tcol, tpoint, alpha, da, db), compose_id(c))
    if f == F252 and c.log_n >= 6:
        check_compose_252_identity(c.log_n, got, base, points, tcol, tpoint, alpha, ood, da, db)
    if c.special == "nterms0":
        assert not got.any(), "no terms: the output is all zero"
    for b, w in zip(B + E, base + ext):
        same(b.read(), w, "an input column after the call")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", COMPOSE, ids=[compose_id(c) for c in COMPOSE])
def test_compose(kind, case):
    run_compose(backends.planner(kind), case, 7000 + 13 * COMPOSE.index(case))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", (FP, FQ3), ids=["fp", "fq3"])
def test_compose_many_terms_on_one_column(kind, field):
    """eight points of 40 terms each over two columns: 160 terms name each column, more than any case of test_compose gives one column (40)
    and more than the 64 that the C oracle's division takes in one pass.  The device, cref.deep_compose and Python integers agree on every word"""
    pl, n, seed = backends.planner(kind), 64, 9100 + field
    h, off = offset_of(field, 1)
    base, ext = [column(FP, n, "mix", seed)], [column(field, n, "mix", seed + 1)]
    if field == FP:
        base, ext = base + ext, []
    tcol, tpoint, alpha, _ = terms_of(field, [40] * 8, 2, None, seed + 50)
    assert min(tcol.count(0), tcol.count(1)) > 64
    points = points_of(field, 8, point_kinds(field, ("rand", "zero", "x", "base")), h, n, seed + 60)
    da, db = degree_of(field, "rand", seed + 70)
    ood = oods_gl(field, base, ext, points, tcol, tpoint)
    B, E, out = [Buf(pl, w) for w in base], [Buf(pl, w) for w in ext], Buf.junk(pl, n * PW[field])
    rc = call_deep(pl, "compose", field, (6, off), B, E, points, tcol, tpoint, alpha, ood, da, db, out.ptr)
    assert rc == MS_OK, pl.lib.ms_last_error().decode()
    pl.sync()
    got = out.read()
    same(got, py_compose_gl(field, n, base, ext, points, tcol, tpoint, alpha, da, db), "against Python integers")
    same(got, ref_compose_gl(field, n, base, ext, points, tcol, tpoint, alpha, da, db), "against cref.deep_compose")
    for b, w in zip(B + E, base + ext):
        same(b.read(), w, "an input column after the call")


# ------------------------------------------------------------------------------------------------------------------
# ms_horner_eval
# ------------------------------------------------------------------------------------------------------------------
H_PAIRS = [(FP, FP), (FP, FQ3), (FQ3, FQ3), (F252, F252)]
H_LENGTHS = [0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 8191, 3 * 4096 + 1] + [5 * 4096 + r for r in (0, 1, 255, 257, 4095)]    # the last five: two levels
Horner = collections.namedtuple("Horner", "cf pf n qkind")


def _horner_cases():
    out = []
    for pi, (cf, pf) in enumerate(H_PAIRS):
        for ni, n in enumerate(H_LENGTHS):
            out.append(Horner(cf, pf, n, "runs"))
        out.append(Horner(cf, pf, 257, "cols96"))
        out.append(Horner(cf, pf, 4097, "cols96"))
        out.append(Horner(cf, pf, 300, "nq0"))
    return out


HORNER = _horner_cases()


def horner_id(c):
    return f"{FNAME[c.cf]}x{FNAME[c.pf]}-n{c.n}-{c.qkind}"


def query_points(pf, nq, seed):
    """points 0, 1, p - 1, the word p - 1, over Fq3 a base-valued point and (0, 1, 0), random ones between them"""
    pw = PW[pf]
    if nq == 0:
        return np.zeros(0, dtype=np.uint64)
    pts = words(pf, nq, seed).reshape(-1, pw)
    if pf == F252:
        fixed = [M252.words([0]), np.array(cref.F252_ONE_MONT, dtype=np.uint64), M252.words([B252.to_mont(P252 - 1)]), M252.words([P252 - 1])]
    else:
        e = lambda *w: np.array(list(w) + [0] * (pw - len(w)), dtype=np.uint64)[:pw]
        fixed = [e(0), e(ONE_GL), e(G.to_mont(P - 1)), e(P - 1)] + ([e(int(pts[0][0])), e(0, ONE_GL, 0), e(P - 1, P - 1, P - 1)] if pw == 3 else [])
    for i, v in enumerate(fixed):
        if 2 * i < nq:
            pts[2 * i] = v
    return np.ascontiguousarray(pts.reshape(-1))


def horner_queries(kind, ncols):
    if kind == "runs":          # same-column runs of 1, 2, 3, 4 and 5 queries (groups of GQ = 2: 1, 2, 2+1, 2+2, 2+2+1), then columns seen before, apart
        return [0] + [1] * 2 + [2] * 3 + [3] * 4 + [4] * 5 + [0, 5, 2, 5]
    if kind == "cols96":
        return list(range(ncols))
    return []


def run_horner(pl, c, seed):
    ncols = 96 if c.qkind == "cols96" else 6
    kinds = ["mix", "mix", "pm1", "zero", "mix", "mix"]
    cols = [column(c.cf, c.n, kinds[i % 6] if i < 6 else "mix", seed + i) for i in range(ncols)]
    qcol = horner_queries(c.qkind, ncols)
    check_horner(pl, c.cf, c.pf, c.n, cols, qcol, query_points(c.pf, len(qcol), seed + 200), what=horner_id(c))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", HORNER, ids=[horner_id(c) for c in HORNER])
def test_horner(kind, case):
    run_horner(backends.planner(kind), case, 9000 + 17 * HORNER.index(case))


THREE = [pytest.param(k, n, id=f"{k}-n{n}", marks=[pytest.mark.gpu] if k == "hip" else [])
         for n in (4096 * 4096 - 1, 4096 * 4096, 4096 * 4096 + 1) for k in (("emu", "hip") if n == 4096 * 4096 + 1 else ("hip",))]


@pytest.mark.parametrize("kind,n", THREE)
def test_horner_three_levels(kind, n):
    """just below, at and above 4096^2 coefficients (two, two and three levels): a column that is zero but at the edges of its blocks, against
    sum c_i x^i in Python integers; Fp points, and Fq3 points (one of them base-valued) for the same column."""
    pl = backends.planner(kind)
    rng = np.random.default_rng(n % 1000)
    pos = sorted(set(p for p in [0, 1, 4095, 4096, 4096 * 4095, 4096 * 4095 + 1, 4096 * 4096 - 2, 4096 * 4096 - 1, 4096 * 4096, n - 1] +
                     [int(x) for x in rng.integers(0, n, size=8)] if p < n))
    vals = [int(v) for v in gl_values(len(pos) + 1, 1, 5)[:len(pos)]]
    col = np.zeros(n, dtype=np.uint64)
    col[pos] = vals
    buf = Buf(pl, col)
    cv = [G.from_mont(v) for v in vals]
    for pf in (FP, FQ3):
        pw = PW[pf]
        pts = query_points(pf, 2, 31 + pw).reshape(-1, pw)
        pts[0] = words(pf, 2, 77)[:pw]
        if pw == 3:
            pts[1] = (int(pts[0][0]), 0, 0)
        want = []
        for z in pts:
            if pw == 1:
                x = G.from_mont(int(z[0]))
                want.append(G.to_mont(sum(c * pow(x, i, P) for i, c in zip(pos, cv)) % P))
            else:
                x, acc = Q3.from_mont(tuple(int(w) for w in z)), (0, 0, 0)
                for i, c in zip(pos, cv):
                    acc = Q3.add(acc, Q3.mul_base(Q3.pow(x, i), c))
                want += list(Q3.to_mont(acc))
        out = np.concatenate([np.full(2 * pw, SENTINEL, dtype=np.uint64), GUARD])
        assert call_horner(pl, FP, pf, n, [buf, buf], [0, 1], np.ascontiguousarray(pts.reshape(-1)), out) == MS_OK
        assert np.array_equal(out[2 * pw:], GUARD)
        same(out[:2 * pw], np.array(want, dtype=np.uint64), f"n = {n}, {FNAME[pf]} points")
    same(buf.read(), col, "the column after the calls")


# ------------------------------------------------------------------------------------------------------------------
# the table of launches
# ------------------------------------------------------------------------------------------------------------------
def test_the_table_names_every_launch():
    """every kernel that a hipLaunchKernelGGL of ms_deep.cpp names is in the table of this file's docstring, and the cases reach every
    dispatch branch at a ragged count on both sides of its thresholds."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ministark_amd", "csrc", "ms_deep.cpp")).read()
    launched = set(re.sub(r"\s", "", m).replace("msdeep::MAXPOINTS", "8").replace("GQ", "2").replace("<R,W>", "<4,4>").strip("()")
                   for m in re.findall(r"hipLaunchKernelGGL\(\(?\s*(ms[a-z0-9]*::[a-z_0-9]+(?:<[^>]*>)?)", src))
    table = {"msdeep::horner_blocks<1,1,2>", "msdeep::horner_blocks<1,3,2>", "msdeep::horner_blocks<3,3,2>", "msdeep252::horner_blocks",
             "msdeep::deep_points<1,4,3>", "msdeep::deep_points<1,2,3>", "msdeep::deep_points<1,1,8>", "msdeep::deep_points<3,2,4>",
             "msdeep::deep_points<3,1,8>", "msdeep::deep_degree_adjust<1>", "msdeep::deep_degree_adjust<3>", "msdeep252::deep_points",
             "msdeep252::deep_degree_adjust", "msdeep252::deep_rows<4,4>"}
    assert launched == table, launched ^ table
    assert all(name.replace("msdeep::", "").replace("msdeep252::", "") in __doc__ for name in table)
    both = lambda c: c.kinds == ("emu", "hip")
    shapes = collections.defaultdict(list)
    for c in ROWS:
        shapes[rows_shape(c.field, c.np, c.count)].append(c)
    for name in ("msdeep::deep_points<1,2,3>", "msdeep::deep_points<3,2,4>", "msdeep::deep_points<1,1,8>", "msdeep::deep_points<3,1,8>", "msdeep252::deep_rows<4,4>"):
        mine = shapes[name]
        assert any(both(c) and c.count >= 4096 and c.count % 512 for c in mine), name                 # ragged against NT * PTS, 4096 rows or more
        assert any(both(c) and c.count < 4096 and c.count % 256 for c in mine) or "<1,2,3>" in name or "<3,2,4>" in name, name
        assert any(c.first % 2 for c in mine) and any(c.first == 0 for c in mine), name
    for f in FIELDS:
        mine = [c for c in ROWS if c.field == f]
        assert set(COUNTS) <= {c.count for c in mine} and {1, 2, 11, 12, 13} <= {c.ld for c in mine}
        assert {c.np for c in mine} == set(range(1, 9)) and {c.offset for c in mine} == set(OFFSETS) and {c.degree for c in mine} == set(DEGREES)
        lo = 3 if f != FQ3 else 4
        assert {lo, lo + 1, 8} <= {c.np for c in mine if c.count >= 4096 and c.count % 512}
        assert {c.first for c in mine if c.ld == LOG_MAIN} >= {0, 1, 777} and any(c.first + c.count == 1 << c.ld and c.first for c in mine)
    assert set(COUNTS252) <= {c.count for c in ROWS if c.field == F252}
    cshapes = {compose_shape(c.field, c.np, 1 << c.log_n): c for c in COMPOSE}
    assert set(cshapes) == {"msdeep252::deep_points", "msdeep::deep_points<1,4,3>", "msdeep::deep_points<1,1,8>", "msdeep::deep_points<3,2,4>", "msdeep::deep_points<3,1,8>"}
    for f in FIELDS:
        for np_ in ((3, 5) if f != FQ3 else (4, 6)):
            assert {c.log_n for c in COMPOSE if c.field == f and c.np == np_ and c.special is None} >= {2, 8, 11, 12, 13}
    for cf, pf in H_PAIRS:
        assert [c.n for c in HORNER if (c.cf, c.pf, c.qkind) == (cf, pf, "runs")] == H_LENGTHS


# ------------------------------------------------------------------------------------------------------------------
# refusals: host-side only, each returns before anything is enqueued; the sentinel-filled output stays as it was
# ------------------------------------------------------------------------------------------------------------------
def _deep_setup(pl, field, n, np_=2, seed=5):
    c = Rows(field, 8, 0, n, np_, None, "rand", (), None, None)
    base, ext, points, tcol, tpoint, alpha, ood, da, db = rows_inputs(c, seed)
    return dict(base=[Buf(pl, w) for w in base], ext=[Buf(pl, w) for w in ext], points=points, tcol=tcol, tpoint=tpoint, alpha=alpha, ood=ood, da=da, db=db,
                words=base + ext)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
@pytest.mark.parametrize("entry", ["rows", "compose"])
def test_deep_refusals_write_nothing(kind, field, entry):
    pl = backends.planner(kind)
    L, n, pw = pl.lib, 256, PW[field]
    s = _deep_setup(pl, field, n)
    sentinel = np.arange(n * pw, dtype=np.uint64) + 17
    out = Buf(pl, sentinel)
    head = (8, None, 0, n) if entry == "rows" else (8, None)

    def call(code, needle, head=head, **kw):
        a = dict(s)
        a.pop("words")
        extra = {k: kw.pop(k) for k in list(kw) if k in ("npoints", "nbase", "next_", "base_table", "ext_table")}
        a.update(kw)
        rc = call_deep(pl, entry, field, head, a["base"], a["ext"], a["points"], a["tcol"], a["tpoint"], a["alpha"], a["ood"], a["da"], a["db"], out.ptr, **extra)
        assert rc == code and needle in L.ms_last_error().decode(), (rc, needle, L.ms_last_error().decode())

    call(MS_ERR_UNSUPPORTED, "distinct out-of-domain points", npoints=0)
    nine = np.concatenate([s["points"]] * 5)[:9 * pw]
    call(MS_ERR_UNSUPPORTED, "distinct out-of-domain points", points=nine, npoints=9)
    many = (VP * 97)(*[s["base"][0].ptr] * 97)                               # 97 columns of a kind: the table is valid, the count is refused
    call(MS_ERR_UNSUPPORTED, "at most 96 columns", base_table=many, nbase=97)
    if field == FQ3:
        many3 = (VP * 97)(*[s["ext"][0].ptr] * 97)
        call(MS_ERR_UNSUPPORTED, "at most 96 columns", ext_table=many3, next_=97)
    else:
        x = Buf(pl, np.zeros(3 * n, dtype=np.uint64))
        call(MS_ERR_INVALID, "extension columns", ext=[x])
    call(MS_ERR_INVALID, "out of range", tcol=[len(s["words"])] + s["tcol"][1:])
    call(MS_ERR_INVALID, "out of range", tpoint=[2] + s["tpoint"][1:])
    # a point on the coset: h w^5 of the call's own domain
    F, h = (B252, 3) if field == F252 else (G, 7)
    z = h * pow(F.root_of_unity(256), 5, F.p) % F.p
    zw = M252.words([F.to_mont(z)]) if field == F252 else u64([F.to_mont(z)] + [0] * (pw - 1))
    call(MS_ERR_INVALID, "lies on", points=np.concatenate([s["points"][:pw], zw]))
    zero_off = np.zeros(pw, dtype=np.uint64)
    call(MS_ERR_INVALID, "offset", head=(head[0], zero_off) + head[2:])
    if entry == "rows":
        call(MS_ERR_INVALID, "outside the domain", head=(8, None, 1, n))
        call(MS_ERR_INVALID, "outside the domain", head=(8, None, n + 1, 0))
        call(MS_ERR_INVALID, "domain of 2^0", head=(0, None, 0, 1))
        call(MS_ERR_INVALID, "domain of 2^33", head=(33, None, 0, 1))
    else:
        call(MS_ERR_INVALID, "log_n too large", head=(41, None))
    pl.sync()
    same(out.read(), sentinel, "the output of the refused calls")
    for b, w in zip(s["base"] + s["ext"], s["words"]):
        same(b.read(), w, "an input of the refused calls")


@pytest.mark.parametrize("kind", KINDS)
def test_horner_refusals_write_nothing(kind):
    pl = backends.planner(kind)
    L, n = pl.lib, 300
    col = Buf(pl, words(F252, n, 3))
    sentinel = np.arange(16, dtype=np.uint64) + 99
    out = sentinel.copy()
    pts = words(F252, 4, 4)
    for cf, pf, code, needle in ((FQ3, FP, MS_ERR_UNSUPPORTED, "embed"), (F252, FP, MS_ERR_UNSUPPORTED, "252-bit"), (FP, F252, MS_ERR_UNSUPPORTED, "252-bit"),
                                 (FQ3, F252, MS_ERR_UNSUPPORTED, "252-bit")):
        assert call_horner(pl, cf, pf, n, [col], [0, 0], pts, out) == code and needle in L.ms_last_error().decode()
    for cf, pf in H_PAIRS:
        assert call_horner(pl, cf, pf, n, [col, col], [0, 2], pts, out) == MS_ERR_INVALID and "names column 2 of 2" in L.ms_last_error().decode()
        assert call_horner(pl, cf, pf, n, [col] * 97, [0], pts, out) == MS_ERR_UNSUPPORTED and "at most 96 columns" in L.ms_last_error().decode()
        assert call_horner(pl, cf, pf, n, [col], [], pts, out) == MS_OK                                   # nq = 0: nothing to do
    assert np.array_equal(out, sentinel)
    same(col.read(), words(F252, n, 3), "the column of the refused calls")


# ------------------------------------------------------------------------------------------------------------------
# aliasing: d_out must not overlap an input column (include/ministark_hip.h)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", FIELDS, ids=[FNAME[f] for f in FIELDS])
@pytest.mark.parametrize("entry", ["rows", "compose"])
def test_an_output_that_overlaps_an_input_column_is_refused(kind, field, entry):
    pl = backends.planner(kind)
    L, n, pw = pl.lib, 256, PW[field]
    s = _deep_setup(pl, field, n)
    head = (8, None, 0, n) if entry == "rows" else (8, None)
    name = "ms_deep_rows" if entry == "rows" else "ms_deep_compose"
    # one arena: [ margin | column | margin ]; the column stands in for the last base column (and, over Fq3, for the last extension column)
    margin = n * pw
    for which in (["base"] if field != FQ3 else ["base", "ext"]):
        colw = s["words"][len(s["base"]) - 1] if which == "base" else s["words"][-1]
        before = np.concatenate([np.full(margin, 0x1111, dtype=np.uint64), colw, np.full(margin, 0x2222, dtype=np.uint64)])
        arena = Buf(pl, before)
        col_at = arena.ptr + 8 * margin
        table = lambda bufs, at: (VP * len(bufs))(*([b.ptr for b in bufs[:-1]] + [at]))
        kw = dict(base_table=table(s["base"], col_at)) if which == "base" else dict(ext_table=table(s["ext"], col_at))
        col_bytes, out_bytes = colw.size * 8, n * pw * 8
        for what, out_at in (("the same address", col_at), ("one word in", col_at + 8), ("its last word", col_at + col_bytes - 8),
                             ("ends one word inside", col_at - out_bytes + 8), ("one element before", col_at - 8 * pw)):
            rc = call_deep(pl, entry, field, head, s["base"], s["ext"], s["points"], s["tcol"], s["tpoint"], s["alpha"], s["ood"], s["da"], s["db"], out_at, **kw)
            msg = L.ms_last_error().decode()
            assert rc == MS_ERR_INVALID and "overlap" in msg and name in msg, (which, what, rc, msg)
        pl.sync()
        same(arena.read(), before, "the arena after the refused calls")
        # allowed: the output ends where the column begins, and begins where it ends
        for out_at in (col_at - out_bytes, col_at + col_bytes):
            assert call_deep(pl, entry, field, head, s["base"], s["ext"], s["points"], s["tcol"], s["tpoint"], s["alpha"], s["ood"], s["da"], s["db"], out_at, **kw) == MS_OK
        pl.sync()
        after = arena.read()
        same(after[margin:margin + colw.size], colw, "the column between two outputs")
        same(after[:margin], after[margin + colw.size:], "the two adjacent outputs")
        assert not np.array_equal(after[:margin], before[:margin])
