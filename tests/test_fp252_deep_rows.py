"""ms_deep_rows over the 252-bit field: the DEEP composition polynomial's values on rows of the bit-reversed LDE domain, computed from
those rows of the committed LDE columns.  Checked word for word against into_deep_poly + bit_reversed_evaluate (both exist and are
tested without this entry point), against the defining formula in Python integers, on row shards, and on its refusals."""
import ctypes
import functools

import numpy as np
import pytest

from oracle.pyref.fields import F252
from tests import backends
from ministark_amd import STARK252_FP, Matrix, Radix2EvaluationDomain, f252_from_mont_limbs, f252_to_mont_limbs
from ministark_amd._lib import MsError
from ministark_amd.api import GpuVec
from ministark_amd.composer import DeepCompositionCoeffs, DeepPolyComposer

P = F252.p
H = 3                                  # the field's generator: the default LDE offset
BLOWUP = 4
KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
ARGS = [(0, 0), (0, 1), (1, 0), (2, 1), (2, -1)]          # offsets -1, 0, 1: the points z / g, z, z g
NBASE, NCOMP = 3, 2
MS_ERR_INVALID = -1


def _rnd(rng):
    return int.from_bytes(rng.bytes(32), "little") % P


def _mat(pl, cols):
    return Matrix.from_numpy(pl, [np.concatenate([f252_to_mont_limbs(v) for v in c]) for c in cols], STARK252_FP)


def _canon(words):
    w = np.asarray(words, dtype=np.uint64).reshape(-1, 4)
    return [f252_from_mont_limbs(r) for r in w]


def _bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def _horner(c, x):
    return functools.reduce(lambda acc, v: (acc * x + v) % P, reversed(c), 0)


def _on_coset(z, N):
    return z % P != 0 and pow(z * pow(H, -1, P) % P, N, P) == 1


def _setup(pl, log_n, seed, beta_zero=False, ncomp=NCOMP):
    """Random polynomials, a composer over them and its coefficients.  With ncomp = 1 the composition point z^1 is z itself: the
    points are z, z g, z / g -- three; with two composition columns z^2 makes a fourth."""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    N = n * BLOWUP
    polys = [[_rnd(rng) for _ in range(n)] for _ in range(NBASE + ncomp)]
    g = F252.root_of_unity(n)
    while True:
        z = _rnd(rng)
        pts = [z, z * g % P, z * pow(g, -1, P) % P, pow(z, ncomp, P)]
        if not any(_on_coset(q, N) for q in pts):
            break
    assert not any(_on_coset(q, N) for q in pts)           # the case below is never an accidental refusal
    bm, cm = _mat(pl, polys[:NBASE]), _mat(pl, polys[NBASE:])
    composer = DeepPolyComposer(ARGS, n, z, bm, None, cm)
    composer.get_ood_evals()
    co = DeepCompositionCoeffs([_rnd(rng) for _ in ARGS], [_rnd(rng) for _ in range(ncomp)], (_rnd(rng), 0 if beta_zero else _rnd(rng)))
    dom = Radix2EvaluationDomain(N, H, STARK252_FP)
    return dict(n=n, N=N, polys=polys, z=z, g=g, bm=bm, cm=cm, composer=composer, co=co, dom=dom, ncomp=ncomp)


def _cases():
    # 2^6 and 2^8 under the simulator, 2^13 on the device; beta zero and non-zero; two composition columns (z^2: a fourth point) and one
    out = []
    for kind, logs in (("emu", (6, 8)), ("hip", (13,))):
        for log_n in logs:
            for beta_zero, ncomp in ((False, 2), (True, 2), (False, 1)):
                out.append(pytest.param(kind, log_n, beta_zero, ncomp, id=f"{kind}-{log_n}-{int(beta_zero)}-{ncomp}",
                                        marks=[pytest.mark.gpu] if kind == "hip" else []))
    return out


@pytest.mark.parametrize("kind,log_n,beta_zero,ncomp", _cases())
def test_rows_equal_deep_poly_then_lde(kind, log_n, beta_zero, ncomp):
    """3 base + composition columns, trace arguments at offsets -1, 0, 1 (ncomp = 1: exactly three distinct points), beta zero and
    non-zero: every row of the LDE domain."""
    pl = backends.planner(kind)
    s = _setup(pl, log_n, 100 + log_n + ncomp, beta_zero, ncomp)
    want = Matrix([s["composer"].into_deep_poly(s["co"])]).bit_reversed_evaluate(s["dom"]).columns[0].to_numpy()
    bl, cl = s["bm"].bit_reversed_evaluate(s["dom"]), s["cm"].bit_reversed_evaluate(s["dom"])
    got = s["composer"].into_deep_evaluations(s["co"], bl, None, cl, s["N"]).to_numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want)


@pytest.mark.parametrize("kind", KINDS)
def test_rows_equal_the_formula_in_integers(kind):
    """(alpha + beta x) sum_k 1/(x - z_k) sum_{t: point_t = k} alpha_t (P_ct(x) - ood_t) with pow(., -1, p), at 64 seeded rows and rows 0, 1, N - 1."""
    pl = backends.planner(kind)
    log_n = 6 if kind == "emu" else 13
    s = _setup(pl, log_n, 7)
    N, n, z, g, polys, co = s["N"], s["n"], s["z"], s["g"], s["polys"], s["co"]
    bl, cl = s["bm"].bit_reversed_evaluate(s["dom"]), s["cm"].bit_reversed_evaluate(s["dom"])
    got = _canon(s["composer"].into_deep_evaluations(co, bl, None, cl, N).to_numpy())
    cols = [_canon(c) for c in bl.to_numpy()] + [_canon(c) for c in cl.to_numpy()]
    z_n = pow(z, NCOMP, P)
    point = lambda off: z * pow(g, off % n, P) % P
    terms = [(NBASE + c, z_n, co.composition_trace[c]) for c in range(NCOMP)] + [(c, point(o), a) for (c, o), a in zip(ARGS, co.execution_trace)]
    terms = [(c, zt, a, _horner(polys[c], zt)) for c, zt, a in terms]            # + the out-of-domain value
    w = F252.root_of_unity(N)
    log_N = N.bit_length() - 1
    rows = sorted(set([0, 1, N - 1] + [int(r) for r in np.random.default_rng(64).integers(0, N, size=64)]))
    for row in rows:
        x = H * pow(w, _bitrev(row, log_N), P) % P
        by_point = {}
        for c, zt, a, ood in terms:
            by_point[zt] = (by_point.get(zt, 0) + a * (cols[c][row] - ood)) % P
        val = sum(v * pow(x - zt, -1, P) for zt, v in by_point.items()) % P
        assert got[row] == val * (co.degree[0] + co.degree[1] * x) % P, row


@pytest.mark.parametrize("kind", KINDS)
def test_row_shards_equal_slices_of_the_whole(kind):
    """The same words for every split of the domain: the shared inversions group other rows in every shard."""
    pl = backends.planner(kind)
    log_n = 8 if kind == "emu" else 13
    s = _setup(pl, log_n, 21)
    N, co = s["N"], s["co"]
    bl, cl = s["bm"].bit_reversed_evaluate(s["dom"]), s["cm"].bit_reversed_evaluate(s["dom"])
    whole = s["composer"].into_deep_evaluations(co, bl, None, cl, N).to_numpy()
    bw, cw = bl.to_numpy(), cl.to_numpy()
    for first, count in ((0, N), (N // 4, N // 4), (N - 64, 64), (5, 1), (N // 2 + 3, 0)):
        if count == 0:
            # a matrix of no rows cannot be built: the entry point itself, with a sentinel in the output
            out = GpuVec.from_numpy(pl, np.full(4, 0xABCD, dtype=np.uint64), STARK252_FP)
            assert _raw(pl, s, first, 0, bl, cl, out) == 0
            assert np.array_equal(out.to_numpy(), np.full(4, 0xABCD, dtype=np.uint64))
            continue
        sl = lambda cols: Matrix.from_numpy(pl, [c[4 * first:4 * (first + count)] for c in cols], STARK252_FP)
        got = s["composer"].into_deep_evaluations(co, sl(bw), None, sl(cw), N, first=first).to_numpy()
        assert np.array_equal(got, whole[4 * first:4 * (first + count)]), (first, count)
    # for_row_shards: the composer of a rank that holds no polynomial, only the gathered out-of-domain values
    rank = DeepPolyComposer.for_row_shards(ARGS, s["n"], s["z"], pl, NBASE, 0, NCOMP, s["composer"]._ood, base_field=STARK252_FP)
    first, count = N // 4, N // 4
    sl = lambda cols: Matrix.from_numpy(pl, [c[4 * first:4 * (first + count)] for c in cols], STARK252_FP)
    got = rank.into_deep_evaluations(co, sl(bw), None, sl(cw), N, first=first, offset=H).to_numpy()
    assert np.array_equal(got, whole[4 * first:4 * (first + count)])


def _raw(pl, s, first, count, bl, cl, out, next_=0, z=None, offset_words=None, log_domain=None):
    """ms_deep_rows itself; returns its status"""
    L = pl.lib
    VP = ctypes.c_void_p
    z = s["z"] if z is None else z
    flat = lambda qs: np.concatenate([f252_to_mont_limbs(q % P) for q in qs]).astype(np.uint64)
    points = [z, z * s["g"] % P]
    tcol, tpoint = [0, 1, 3], [0, 1, 0]
    pts, al, od = flat(points), flat([5, 6, 7]), flat([8, 9, 10])
    da, db = flat([11]), flat([12])
    cols = [c.ptr for c in list(bl.columns) + list(cl.columns)]
    ext = [cols[-1]] * max(1, next_)
    off = None if offset_words is None else offset_words.ctypes.data
    return L.ms_deep_rows(pl.handle, STARK252_FP, (s["N"].bit_length() - 1) if log_domain is None else log_domain, off, first, count,
                          (VP * len(cols))(*cols), len(cols), (VP * len(ext))(*ext), next_, pts.ctypes.data, len(points),
                          (ctypes.c_uint * 3)(*tcol), (ctypes.c_uint * 3)(*tpoint), al.ctypes.data, od.ctypes.data, 3,
                          da.ctypes.data, db.ctypes.data, out.ptr)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_write_nothing(kind):
    pl = backends.planner(kind)
    s = _setup(pl, 6, 33)
    N = s["N"]
    bl, cl = s["bm"].bit_reversed_evaluate(s["dom"]), s["cm"].bit_reversed_evaluate(s["dom"])
    sentinel = np.arange(4 * N, dtype=np.uint64) + 17
    out = GpuVec.from_numpy(pl, sentinel, STARK252_FP)
    assert _raw(pl, s, 0, N, bl, cl, out, next_=1) == MS_ERR_INVALID                                 # an extension column
    w = F252.root_of_unity(N)
    assert _raw(pl, s, 0, N, bl, cl, out, z=H * pow(w, 5, P) % P) == MS_ERR_INVALID                   # a point on the LDE coset
    p_words = np.array([P >> (64 * i) & (2 ** 64 - 1) for i in range(4)], dtype=np.uint64)
    assert _raw(pl, s, 0, N, bl, cl, out, offset_words=p_words) == MS_ERR_INVALID                     # offset = p: not canonical
    assert _raw(pl, s, 0, N, bl, cl, out, offset_words=np.zeros(4, dtype=np.uint64)) == MS_ERR_INVALID
    assert _raw(pl, s, N - 8, 9, bl, cl, out) == MS_ERR_INVALID                                       # rows past the domain
    assert _raw(pl, s, N + 1, 0, bl, cl, out) == MS_ERR_INVALID
    assert np.array_equal(out.to_numpy(), sentinel)
    assert _raw(pl, s, 0, N, bl, cl, out) == 0                                                        # and the same call, legal, runs
    assert not np.array_equal(out.to_numpy(), sentinel)
    with pytest.raises(MsError, match="coset"):                                                       # the binding reports it
        c = DeepPolyComposer(ARGS, s["n"], H * pow(w, 5, P) % P, s["bm"], None, s["cm"])
        c.into_deep_evaluations(s["co"], bl, None, cl, N)
