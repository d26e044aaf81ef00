#!/usr/bin/env python3
"""Randomised differential run of the library against the C oracle (oracle/c) on the GPU:
    python tests/fuzz_parity.py [seconds] [seed]
Random sizes (2^0 .. 2^21: every plan family incl. the (256, R, 256) ones), fields, directions, coset offsets, blow-ups, folding factors, shifts and column
counts; the element-wise stages run through the C ABI at any length up to 2^15, not only powers of two; the DEEP entry points (ms_deep_rows, ms_deep_compose,
ms_horner_eval) through the C ABI over all three fields with any number of points, 0..40 terms per point and any first / count up to 2^13; values are a mix of uniform elements and edge values (0, 1, p-1, 2^32-1, 2^32, p-2^32 ...).
Complements tests/ (fixed shapes): any mismatch prints the failing case and exits non-zero.  MS_FUZZ_BACKEND=emu: the same on the simulator build
(CPU; transforms to 2^18, LDEs to 2^14 rows)."""
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from oracle import cref  # noqa: E402  (the checker)
from ministark_amd import (GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, GpuFft, GpuIfft, GpuVec, Matrix, MerkleTree, Planner,  # noqa: E402
                           Radix2EvaluationDomain, apply_drp, gl_to_mont)
from ministark_amd import stages as S  # noqa: E402

P = cref.GL_P
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(seed)
EMU = __import__("os").environ.get("MS_FUZZ_BACKEND") == "emu"      # the simulator build (CPU): the same kernels, smaller upper sizes
if EMU:
    from tests import backends  # noqa: E402
    pl = backends.planner("emu")
else:
    pl = Planner(0)
TOP_NTT, TOP_LDE = (19, 15) if EMU else (22, 18)
EDGE = np.array([gl_to_mont(v % P) for v in (0, 1, 2, P - 1, P - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - (1 << 32), (1 << 63), 7)], dtype=np.uint64)
RAW_EDGE = np.array([0, 1, P - 1, P - 2, 0xFFFFFFFF, 1 << 32, 0xFFFFFFFF00000000], dtype=np.uint64)   # canonical Montgomery words


def values(n_words):
    a = rng.integers(0, P, size=n_words, dtype=np.uint64)
    mode = rng.integers(0, 4)
    if mode == 1:
        m = rng.random(n_words) < 0.3
        a[m] = rng.choice(np.concatenate([EDGE, RAW_EDGE]), size=int(m.sum()))
    elif mode == 2:
        a[:] = rng.choice(np.concatenate([EDGE, RAW_EDGE]), size=n_words)
    return a


def offset():
    return int(rng.choice([1, 7, 3, P - 1, int(rng.integers(2, 1 << 62))]))


def case_ntt():
    log_n, V, inv, off = int(rng.integers(0, TOP_NTT)), int(rng.choice([1, 3])), bool(rng.integers(0, 2)), offset()
    field = FQ3 if V == 3 else FP
    x = values((1 << log_n) * V)
    v = GpuVec.from_numpy(pl, x, field)
    f = (GpuIfft if inv else GpuFft)(Radix2EvaluationDomain(1 << log_n, off), field, pl)
    f.encode(v); f.execute(); f.close()
    return np.array_equal(v.to_numpy(), cref.ntt(x, log_n, V, inv, off)), f"ntt log_n={log_n} V={V} inv={inv} off={off}"


def case_lde():
    log_n, log_b, V, off, br = int(rng.integers(0, TOP_LDE)), int(rng.integers(0, 6)), int(rng.choice([1, 3])), offset(), bool(rng.integers(0, 2))
    field = FQ3 if V == 3 else FP
    cols = [values((1 << log_n) * V) for _ in range(int(rng.integers(1, 4)))]
    out = Matrix.from_numpy(pl, cols, field).lde(1 << log_b, off, br).to_numpy()
    ok = all(np.array_equal(o, cref.lde(c, log_n, log_b, V, off, br)) for o, c in zip(out, cols))
    return ok, f"lde log_n={log_n} log_b={log_b} V={V} off={off} bit_reversed={br}"


def case_evaluate():
    log_n, log_b, off, br = int(rng.integers(0, 14)), int(rng.integers(0, 6)), offset(), bool(rng.integers(0, 2))
    n, N = 1 << log_n, 1 << (log_n + log_b)
    c = values(n)
    padded = np.zeros(N, dtype=np.uint64); padded[:n] = c
    want = cref.ntt(padded, log_n + log_b, 1, False, off)
    if br:
        want = cref.bit_reverse(want, log_n + log_b, 1)
    m = Matrix.from_numpy(pl, [c], FP)
    got = (m.bit_reversed_evaluate if br else m.evaluate)(Radix2EvaluationDomain(N, off)).to_numpy()[0]
    return np.array_equal(got, want), f"evaluate log_n={log_n} log_b={log_b} off={off} bit_reversed={br}"


def case_fri():
    ff = int(rng.choice([2, 4, 8, 16]))
    log_n, V, off = int(rng.integers(ff.bit_length() - 1, 17)), int(rng.choice([1, 3])), offset()
    field = FQ3 if V == 3 else FP
    ev, alpha = values((1 << log_n) * V), values(V)
    got = apply_drp(GpuVec.from_numpy(pl, ev, field), alpha, ff, off).to_numpy()
    return np.array_equal(got, cref.fri_fold(ev, log_n, V, ff, alpha, off)), f"fri log_n={log_n} V={V} ff={ff} off={off}"


def case_commit():
    log_n, ncols, V = int(rng.integers(1, 13)), int(rng.integers(1, 40)), int(rng.choice([1, 3]))
    field = FQ3 if V == 3 else FP
    cols = [values((1 << log_n) * V) for _ in range(ncols)]
    tree = MerkleTree.from_matrix(Matrix.from_numpy(pl, cols, field))
    want = cref.sha256_merkle(cref.sha256_rows(cols, V))
    return tree.root() == want[1].tobytes() and np.array_equal(tree.nodes_numpy()[1:], want[1:]), f"commit log_n={log_n} ncols={ncols} V={V}"


def case_stage():
    # through the C ABI, where n is free (the stage wrappers keep the reference's power-of-two rule): any length up to 2^15
    n = int(rng.integers(1, (1 << 15) + 1)) if rng.integers(0, 4) else 1 << int(rng.integers(0, 16))
    lf, rf = [(FP, FP), (FQ3, FQ3), (FQ3, FP)][int(rng.integers(0, 3))]
    VL, VR = (3 if lf == FQ3 else 1), (3 if rf == FQ3 else 1)
    a, b, shift, e = values(n * VL), values(n * VR), int(rng.integers(-2 * n, 2 * n + 1)), int(rng.integers(0, 40))
    A, B, D = GpuVec.from_numpy(pl, a, lf), GpuVec.from_numpy(pl, b, rf), GpuVec(pl, n, lf)
    L, h = pl.lib, pl.handle
    L.check(L.ms_binary(h, S.MUL, lf, rf, n, D.ptr, A.ptr, B.ptr, shift))
    ok = np.array_equal(D.to_numpy(), cref.binary(1, VL, VR, a, b, shift))
    L.check(L.ms_binary(h, S.ADD, lf, rf, n, D.ptr, A.ptr, B.ptr, shift))
    ok &= np.array_equal(D.to_numpy(), cref.binary(0, VL, VR, a, b, shift))
    # the const stages, into another buffer and in place
    c, op = values(VR), int(rng.integers(0, 2))
    L.check(L.ms_binary_const(h, op, lf, rf, n, D.ptr, A.ptr, c.ctypes.data))
    ok &= np.array_equal(D.to_numpy(), cref.binary_const(op, VL, VR, a, c))
    L.check(L.ms_binary_const(h, 1 - op, lf, rf, n, D.ptr, D.ptr, c.ctypes.data))
    ok &= np.array_equal(D.to_numpy(), cref.binary_const(1 - op, VL, VR, cref.binary_const(op, VL, VR, a, c), c))
    L.check(L.ms_mul_pow(h, lf, rf, n, A.ptr, A.ptr, B.ptr, e, shift))
    ok &= np.array_equal(A.to_numpy(), cref.mul_pow(VL, VR, a, b, e, shift))
    L.check(L.ms_unary(h, S.INV, lf, n, D.ptr, A.ptr, 0))
    ok &= np.array_equal(D.to_numpy(), cref.unary(1, VL, A.to_numpy(), 0))
    # ConvertInto (the embedding, or the copy between equal fields), FillBuff, sum_columns (dst is sometimes one of the columns)
    L.check(L.ms_convert(h, lf, rf, n, D.ptr, B.ptr))
    emb = np.zeros((n, VL), dtype=np.uint64)
    emb[:, :VR] = b.reshape(n, VR)
    ok &= np.array_equal(D.to_numpy(), emb.reshape(-1))
    fill = values(VL)
    L.check(L.ms_fill(h, lf, n, D.ptr, fill.ctypes.data))
    ok &= np.array_equal(D.to_numpy(), np.tile(fill, n))
    ncols = int(rng.choice([1, 2, 3, 17, 127, 128]))
    cols = [values(n * VL) for _ in range(min(ncols, 4))]
    vecs = [GpuVec.from_numpy(pl, x, lf) for x in cols]
    idx = [int(k) for k in rng.integers(0, len(cols), size=ncols)]              # columns may alias each other
    dst = vecs[idx[int(rng.integers(0, ncols))]] if rng.integers(0, 2) else D
    arr = (__import__("ctypes").c_void_p * ncols)(*[vecs[k].ptr for k in idx])
    L.check(L.ms_sum_columns(h, lf, n, arr, ncols, dst.ptr))
    ok &= np.array_equal(dst.to_numpy(), cref.sum_columns([cols[k] for k in idx], VL))
    return bool(ok), f"stage n={n} fields=({VL},{VR}) shift={shift} e={e} const_op={op} ncols={ncols}"


def case_deep():
    # the DEEP entry points through the C ABI (tests/deep_ref.py: the references of tests/test_deep_sweep.py): any field, any number of points,
    # 0..40 terms per point, any first / count up to 2^13, edge words at a drawn density
    from tests import deep_ref as D
    f = [D.FP, D.FQ3, D.F252][int(rng.integers(0, 3))]
    entry = ["rows", "compose", "horner"][int(rng.integers(0, 3))]
    npoints, density, seed = int(rng.integers(1, 9)), float(rng.choice([0.0, 0.1, 0.3, 0.9])), int(rng.integers(1 << 30))
    counts = [int(rng.integers(0, 41)) for _ in range(npoints)]
    nbase, next_ = int(rng.integers(0 if f == D.FQ3 else 1, 6)), (int(rng.integers(0, 4)) if f == D.FQ3 else 0)
    if nbase + next_ == 0:
        nbase = 1
    offset, degree = [None, 1, "other"][int(rng.integers(0, 3))], ["rand", "b0", "a0", "one"][int(rng.integers(0, 4))]
    kinds = tuple(str(k) for k in rng.choice(["rand", "zero", "base", "x"] if f == D.FQ3 else ["rand", "zero"], size=2, replace=False))
    bf = D.F252 if f == D.F252 else D.FP
    what = f"deep {entry} field={f} npoints={npoints} counts={counts} nbase={nbase} next={next_} offset={offset} degree={degree} density={density} seed={seed}"
    try:
        if entry == "rows":
            ld = int(rng.integers(1, 15))
            N = 1 << ld
            count = int(rng.integers(1, min(N, 1 << 13) + 1))
            first = int(rng.integers(0, N - count + 1))
            what += f" log_domain={ld} first={first} count={count}"
            h, _ = D.offset_of(f, offset)
            base = [D.column(bf, count, "mix", seed + c, density) for c in range(nbase)]
            ext = [D.column(D.FQ3, count, "mix", seed + 10 + c, density) for c in range(next_)]
            tcol, tpoint, alpha, ood = D.terms_of(f, counts, nbase + next_, None, seed + 50, density)
            points = D.points_of(f, npoints, kinds, h, N, seed + 60)
            da, db = D.degree_of(f, degree, seed + 70)
            D.check_rows(pl, f, ld, first, count, offset, base, ext, points, tcol, tpoint, alpha, ood, da, db, seed, what)
        elif entry == "compose":
            log_n = int(rng.integers(0, 12 if f == D.F252 else 14))
            n = 1 << log_n
            what += f" log_n={log_n}"
            h, off = D.offset_of(f, offset)
            base = [D.column(bf, n, "mix", seed + c, density) for c in range(nbase)]
            ext = [D.column(D.FQ3, n, "mix", seed + 10 + c, density) for c in range(next_)]
            tcol, tpoint, alpha, _ = D.terms_of(f, counts, nbase + next_, None, seed + 50, density)
            points = D.points_of(f, npoints, kinds, h, n, seed + 60)
            da, db = D.degree_of(f, degree, seed + 70)
            ood = D.oods_252(base, points, tcol, tpoint) if f == D.F252 else D.oods_gl(f, base, ext, points, tcol, tpoint)
            B, E, out = [D.Buf(pl, w) for w in base], [D.Buf(pl, w) for w in ext], D.Buf.junk(pl, n * D.PW[f])
            assert D.call_deep(pl, "compose", f, (log_n, off), B, E, points, tcol, tpoint, alpha, ood, da, db, out.ptr) == 0, pl.lib.ms_last_error().decode()
            pl.sync()
            if f != D.F252:
                D.same(out.read(), D.ref_compose_gl(f, n, base, ext, points, tcol, tpoint, alpha, da, db), what)
            elif log_n <= 7:
                D.same(out.read(), D.ref_compose_252_division(n, base, points, tcol, tpoint, alpha, da, db), what)
            elif not any(D.on_coset(f, points[4 * k:4 * k + 4], 5, n) for k in range(npoints)):
                D.check_compose_252_identity(log_n, out.read(), base, points, tcol, tpoint, alpha, ood, da, db)
        else:
            cf, pf = [(D.FP, D.FP), (D.FP, D.FQ3), (D.FQ3, D.FQ3), (D.F252, D.F252)][int(rng.integers(0, 4))]
            n = int(rng.integers(0, (1 << 13) + 1))
            ncols = int(rng.integers(1, 7))
            qcol = sorted(int(c) for c in rng.integers(0, ncols, size=int(rng.integers(0, 12)))) + [int(c) for c in rng.integers(0, ncols, size=3)]
            what = f"deep horner fields=({cf},{pf}) n={n} qcol={qcol} density={density} seed={seed}"
            cols = [D.column(cf, n, "mix", seed + c, density) for c in range(ncols)]
            D.check_horner(pl, cf, pf, n, cols, qcol, D.words(pf, len(qcol), seed + 9, density), what=what)
    except AssertionError as e:
        return False, what + ": " + str(e)[:300]
    return True, what


CASES = [case_ntt, case_lde, case_evaluate, case_fri, case_commit, case_stage, case_deep]
t0, count = time.time(), 0
while time.time() - t0 < budget:
    fn = CASES[int(rng.integers(0, len(CASES)))]
    ok, what = fn()
    count += 1
    if not ok:
        print(f"MISMATCH after {count} cases (seed {seed}): {what}")
        sys.exit(1)
print(f"fuzz ok: {count} random cases in {time.time() - t0:.0f} s (seed {seed})")
