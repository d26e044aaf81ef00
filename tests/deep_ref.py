"""Helpers of tests/test_deep_sweep.py and of the DEEP case of tests/fuzz_parity.py: inputs, the references and the ctypes calls of
ms_deep_rows, ms_deep_compose and ms_horner_eval.  Nothing here shares code with csrc/.

References (words in, words out; Montgomery words as they cross the C ABI):
  rows, Goldilocks   ref_rows_gl: the defining formula assembled from oracle.cref's array operations (binary, binary_const, unary INV --
                     tests/test_stage_sweep.py pins those against big integers); py_rows_gl: the same formula on Python integers
                     (oracle.pyref.fields), row by row -- every checked call compares a seeded sample of its rows with it as well.
  rows, 252-bit      ref_rows_252: Python integers.
  compose            ref_compose_gl: cref.deep_compose (synthetic division per column); py_compose_gl: the same on Python integers, term by
                     term; ref_compose_252_division: synthetic division in Python integers; check_compose_252_identity: the evaluation identity at the n points of a coset.
  horner             ref_horner: cref.horner_eval; Python integers for the 252-bit field; sparse columns: sum c_i x^i."""
import ctypes

import numpy as np

from oracle import cref
from oracle.pyref import fields as PF
from tests.test_stage_sweep import GL_EDGE, GUARD, M252, Buf, gl_values, same
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, STARK252_FP as F252

P = cref.GL_P
P252 = PF.F252_P
PW = {FP: 1, FQ3: 3, F252: 4}
ADD, MUL, INV = 0, 1, 1
MS_OK, MS_ERR_INVALID, MS_ERR_UNSUPPORTED = 0, -1, -2
VP = ctypes.c_void_p
G, Q3, B252 = PF.GL, PF.FQ3, PF.F252
ONE_GL = G.to_mont(1)
TOP252 = (1 << 251) - 1            # the canonical word with the largest digits: eight of 2^28 - 1 and a ninth of 2^27 - 1
SENTINEL = 0xDEADBEEFDEADBEEF


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def u64(xs):
    return np.array(list(xs), dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def words(field, n, seed, density=0.3):
    """n elements of `field`: uniform words with the edge words sprinkled in (gl_values / M252.values); density 0: uniform only"""
    if field == F252:
        if density:
            return M252.values(n, seed)
        a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 59) - 1)
        return a.reshape(-1)
    if density:
        return gl_values(n, PW[field], seed)
    return np.random.default_rng(seed).integers(0, P, size=n * PW[field], dtype=np.uint64)


def column(field, n, kind, seed, density=0.3):
    """kind: mix | pm1 (every Montgomery word p - 1) | zero | top (252-bit: every word 2^251 - 1)"""
    if kind == "zero":
        return np.zeros(n * PW[field], dtype=np.uint64)
    if kind == "pm1":
        return M252.words([P252 - 1] * n) if field == F252 else np.full(n * PW[field], P - 1, dtype=np.uint64)
    if kind == "top":
        return M252.words([TOP252] * n)
    return words(field, n, seed, density)


def offset_of(field, kind):
    """(canonical offset, the words handed to the call or None).  kind: None (the default: 7, or 3), 1, other"""
    default, other = (3, 5) if field == F252 else (7, 11)
    if kind is None:
        return default, None
    h = 1 if kind == 1 else other
    return h, (M252.words([B252.to_mont(h)]) if field == F252 else u64([G.to_mont(h)]))


def on_coset(field, z_words, h, N):
    """does the point lie on h<w_N>?  (only a base-field point can)"""
    if field == F252:
        z = B252.from_mont(M252.ints(z_words)[0])
        return z != 0 and pow(z * pow(h, -1, P252) % P252, N, P252) == 1
    if field == FQ3 and (int(z_words[1]) or int(z_words[2])):
        return False
    z = G.from_mont(int(z_words[0]))
    return z != 0 and pow(z * pow(h, -1, P) % P, N, P) == 1


def points_of(field, npoints, kinds, h, N, seed):
    """npoints distinct points off the coset.  kinds[k]: zero | x (the element (0, 1, 0)) | base (an Fq3 point whose upper components are
    zero) | anything else: random words with edge words"""
    rng = np.random.default_rng(seed)
    pw, out = PW[field], []
    for k in range(npoints):
        kind = kinds[k] if k < len(kinds) else "rand"
        for attempt in range(100):
            z = words(field, 3, int(rng.integers(1 << 30)))[:pw].copy()
            if kind == "zero":
                z[:] = 0
            elif kind == "x":
                z[:] = (0, ONE_GL, 0)
            elif kind == "base" and pw == 3:
                z[1:] = 0
            fixed = not z.any() or (pw == 3 and tuple(int(w) for w in z) == (0, ONE_GL, 0))     # a drawn point never takes a fixed one's place
            if not on_coset(field, z, h, N) and not any(np.array_equal(z, o) for o in out) and (kind in ("zero", "x") or not fixed):
                break
            assert kind not in ("zero", "x"), "a fixed point cannot be drawn again"
        else:
            raise AssertionError("no point off the coset")
        out.append(z)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


def terms_of(field, counts, ncols, skip, seed, density=0.3, heavy=None):
    """counts[k] terms for point k, listed round-robin over the points (so that the caller's order is NOT sorted by point); term columns
    cycle over every column but `skip` (a column no term names; the others are named several times).  Every fifth alpha is p - 1 in every
    word.  heavy = (point, column, alpha words): every term of that point names that column with that alpha.
    -> tcol, tpoint, alpha words, ood words"""
    pw = PW[field]
    left = list(counts)
    usable = [c for c in range(ncols) if c != skip] or [0]
    tcol, tpoint = [], []
    while any(left):
        for k in range(len(left)):
            if left[k]:
                left[k] -= 1
                tpoint.append(k)
                tcol.append(usable[len(tcol) % len(usable)])
    nt = len(tcol)
    alpha, ood = words(field, max(nt, 1), seed, density).reshape(-1, pw), words(field, max(nt, 1), seed + 1, density).reshape(-1, pw)
    for t in range(0, nt, 5):
        alpha[t] = M252.words([P252 - 1]) if field == F252 else P - 1
    if heavy is not None:
        for t in range(nt):
            if tpoint[t] == heavy[0]:
                tcol[t] = heavy[1]
                alpha[t] = heavy[2]
    return tcol, tpoint, np.ascontiguousarray(alpha.reshape(-1)), np.ascontiguousarray(ood.reshape(-1))


def degree_of(field, kind, seed):
    """(a, b) words.  kind: rand | b0 | a0 | one (the pair (1, 0))"""
    pw = PW[field]
    w = words(field, 3, seed).reshape(-1, pw)
    a, b = w[0].copy(), w[1].copy()
    if kind in ("b0", "one"):
        b[:] = 0
    if kind == "a0":
        a[:] = 0
    if kind == "one":
        a[:] = 0
        if field == F252:
            a[:] = cref.F252_ONE_MONT
        else:
            a[0] = ONE_GL
    return a, b


# ------------------------------------------------------------------------------------------------------------------
# references: ms_deep_rows
# ------------------------------------------------------------------------------------------------------------------
def xs_of(field, h, log_domain, first, count):
    """x_i = h w_N^bitrev(first + i), canonical integers, from Python's pow"""
    F = B252 if field == F252 else G
    w = F.root_of_unity(1 << log_domain)
    return [h * pow(w, bitrev(first + i, log_domain), F.p) % F.p for i in range(count)]


def _neg(w):
    return u64((P - int(x)) % P for x in w)


def _embed(col, pw):
    if pw == 1:
        return col
    e = np.zeros((col.size, 3), dtype=np.uint64)
    e[:, 0] = col
    return e.reshape(-1)


def ref_rows_gl(field, xs, base, ext, points, tcol, tpoint, alpha, ood, da, db):
    """(a + b x) sum_k 1/(x - z_k) sum_{t: point_t = k} alpha_t (P_ct(x) - ood_t) over whole columns, from cref's array operations"""
    pw, n, nbase = PW[field], len(xs), len(base)
    xe = _embed(u64(G.to_mont(x) for x in xs), pw)
    add = lambda a, b: cref.binary(ADD, pw, pw, a, b)
    mul = lambda a, b: cref.binary(MUL, pw, pw, a, b)
    addc = lambda a, c: cref.binary_const(ADD, pw, pw, a, c)
    mulc = lambda a, c: cref.binary_const(MUL, pw, pw, a, c)
    total = np.zeros(n * pw, dtype=np.uint64)
    emb = {}
    for k in range(len(points) // pw):
        num = np.zeros(n * pw, dtype=np.uint64)
        mine = [t for t in range(len(tcol)) if tpoint[t] == k]
        for t in mine:
            c = tcol[t]
            if c not in emb:
                emb[c] = _embed(base[c], pw) if c < nbase else ext[c - nbase]
            num = add(num, mulc(addc(emb[c], _neg(ood[t * pw:(t + 1) * pw])), alpha[t * pw:(t + 1) * pw]))
        if mine:
            total = add(total, mul(num, cref.unary(INV, pw, addc(xe, _neg(points[k * pw:(k + 1) * pw])))))
    return mul(total, addc(mulc(xe, db), da))


def py_rows_gl(field, xs, rows, base, ext, points, tcol, tpoint, alpha, ood, da, db):
    """the same formula on Python integers, for the rows listed -> {row: words}"""
    pw, nbase = PW[field], len(base)
    if pw == 1:
        F, lift, get = G, (lambda v: v), (lambda w, i: G.from_mont(int(w[i])))
        put = lambda v: [G.to_mont(v)]
    else:
        F, lift, get = Q3, Q3.embed, (lambda w, i: Q3.from_mont(tuple(int(x) for x in w[3 * i:3 * i + 3])))
        put = lambda v: list(Q3.to_mont(v))
    zero = lift(0)
    zs = [get(points, k) for k in range(len(points) // pw)]
    al, od = [get(alpha, t) for t in range(len(tcol))], [get(ood, t) for t in range(len(tcol))]
    a, b = get(da, 0), get(db, 0)
    out = {}
    for i in rows:
        x = lift(xs[i])
        tot = zero
        for k, z in enumerate(zs):
            num = zero
            for t in range(len(tcol)):
                if tpoint[t] == k:
                    c = tcol[t]
                    v = lift(G.from_mont(int(base[c][i]))) if c < nbase else Q3.from_mont(tuple(int(w) for w in ext[c - nbase][3 * i:3 * i + 3]))
                    num = F.add(num, F.mul(al[t], F.sub(v, od[t])))
            if num != zero:
                tot = F.add(tot, F.mul(num, F.inv(F.sub(x, z))))
        out[i] = put(F.mul(tot, F.add(a, F.mul(b, x))))
    return out


def ref_rows_252(xs, cols, points, tcol, tpoint, alpha, ood, da, db):
    p, fm = P252, B252.from_mont
    C = [[fm(v) for v in M252.ints(c)] for c in cols]
    zs, al, od = [fm(v) for v in M252.ints(points)], [fm(v) for v in M252.ints(alpha)], [fm(v) for v in M252.ints(ood)]
    a, b = fm(M252.ints(da)[0]), fm(M252.ints(db)[0])
    by_point = [[t for t in range(len(tcol)) if tpoint[t] == k] for k in range(len(zs))]
    out = []
    for i, x in enumerate(xs):
        tot = 0
        for k, z in enumerate(zs):
            if by_point[k]:
                tot += sum(al[t] * (C[tcol[t]][i] - od[t]) for t in by_point[k]) % p * pow(x - z, -1, p)
        out.append(B252.to_mont(tot * (a + b * x) % p))
    return M252.words(out)


# ------------------------------------------------------------------------------------------------------------------
# the calls
# ------------------------------------------------------------------------------------------------------------------
def _table(bufs):
    return (VP * len(bufs))(*[b.ptr for b in bufs]) if bufs else None


def _uints(xs):
    return (ctypes.c_uint * max(1, len(xs)))(*xs)


def call_deep(pl, entry, field, head, base, ext, points, tcol, tpoint, alpha, ood, da, db, out_ptr, npoints=None, nbase=None, next_=None,
              base_table=None, ext_table=None):
    """entry: "rows" (head = (log_domain, offset words or None, first, count)) or "compose" (head = (log_n, offset words or None)).
    base / ext: lists of Buf.  -> the status"""
    L = pl.lib
    fn = L.ms_deep_rows if entry == "rows" else L.ms_deep_compose
    head = list(head)
    head[1] = None if head[1] is None else head[1].ctypes.data
    pad = lambda w: w if w.size else np.zeros(4, dtype=np.uint64)
    points, alpha, ood = pad(points), pad(alpha), pad(ood)
    return fn(pl.handle, field, *head, base_table if base_table is not None else _table(base), len(base) if nbase is None else nbase,
              ext_table if ext_table is not None else _table(ext), len(ext) if next_ is None else next_, points.ctypes.data,
              (points.size // PW[field]) if npoints is None else npoints, _uints(tcol), _uints(tpoint), alpha.ctypes.data, ood.ctypes.data, len(tcol),
              da.ctypes.data, db.ctypes.data, out_ptr)


def sample_rows(count, seed, k=6):
    if count <= 8:
        return list(range(count))
    return sorted(set([0, count - 1] + [int(r) for r in np.random.default_rng(seed).integers(0, count, size=k)]))


def check_rows(pl, field, log_domain, first, count, offset_kind, base_w, ext_w, points, tcol, tpoint, alpha, ood, da, db, seed=0, what="rows"):
    """one ms_deep_rows call, every word of it: the output against the reference (and a sample of rows against the formula in Python integers),
    the guard words behind the output, every input column afterwards.  -> the output words"""
    pw = PW[field]
    h, off = offset_of(field, offset_kind)
    base, ext = [Buf(pl, w) for w in base_w], [Buf(pl, w) for w in ext_w]
    out = Buf.junk(pl, count * pw)
    rc = call_deep(pl, "rows", field, (log_domain, off, first, count), base, ext, points, tcol, tpoint, alpha, ood, da, db, out.ptr)
    assert rc == MS_OK, f"{what}: status {rc}: {pl.lib.ms_last_error().decode()}"
    pl.sync()
    got = out.read()
    xs = xs_of(field, h, log_domain, first, count)
    if field == F252:
        want = ref_rows_252(xs, base_w, points, tcol, tpoint, alpha, ood, da, db)
    else:
        want = ref_rows_gl(field, xs, base_w, ext_w, points, tcol, tpoint, alpha, ood, da, db)
        for i, w in py_rows_gl(field, xs, sample_rows(count, seed), base_w, ext_w, points, tcol, tpoint, alpha, ood, da, db).items():
            assert [int(v) for v in want[i * pw:(i + 1) * pw]] == w, f"{what}: the two references differ at row {i}"
    same(got, want, what)
    for b, w in zip(base + ext, list(base_w) + list(ext_w)):
        same(b.read(), w, what + ": an input column after the call")
    return got


# ------------------------------------------------------------------------------------------------------------------
# references: ms_deep_compose
# ------------------------------------------------------------------------------------------------------------------
def oods_gl(field, base_w, ext_w, points, tcol, tpoint):
    """ood_t = P_ct(z_pt): the quotient is a polynomial only then"""
    pw, nbase, memo, out = PW[field], len(base_w), {}, []
    for c, k in zip(tcol, tpoint):
        if (c, k) not in memo:
            memo[(c, k)] = cref.horner_eval(base_w[c] if c < nbase else ext_w[c - nbase], 1 if c < nbase else 3, points[k * pw:(k + 1) * pw])
        out.append(memo[(c, k)])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


def ref_compose_gl(field, n, base_w, ext_w, points, tcol, tpoint, alpha, da, db):
    pw, cols = PW[field], list(base_w) + list(ext_w)
    by_poly = []
    for c in range(len(cols)):
        mine = [t for t in range(len(tcol)) if tcol[t] == c]
        zs = [points[tpoint[t] * pw:(tpoint[t] + 1) * pw] for t in mine]
        cs = [alpha[t * pw:(t + 1) * pw] for t in mine]
        by_poly.append((np.concatenate(zs) if zs else np.zeros(0, dtype=np.uint64), np.concatenate(cs) if cs else np.zeros(0, dtype=np.uint64)))
    return cref.deep_compose(cols, [1] * len(base_w) + [3] * len(ext_w), by_poly, n, pw, (da, db))


def py_compose_gl(field, n, base_w, ext_w, points, tcol, tpoint, alpha, da, db):
    """the same on Python integers (oracle.pyref.fields), term by term: any number of terms on one column"""
    pw, nbase = PW[field], len(base_w)
    if pw == 1:
        F, lift, get, put = G, (lambda v: v), (lambda w, i: G.from_mont(int(w[i]))), (lambda v: [G.to_mont(v)])
    else:
        F, lift, get, put = Q3, Q3.embed, (lambda w, i: Q3.from_mont(tuple(int(x) for x in w[3 * i:3 * i + 3]))), (lambda v: list(Q3.to_mont(v)))
    zero = lift(0)
    acc = [zero] * n
    for t in range(len(tcol)):
        c = tcol[t]
        co = [lift(G.from_mont(int(v))) for v in base_w[c]] if c < nbase else [get(ext_w[c - nbase], i) for i in range(n)]
        z, al, carry = get(points, tpoint[t]), get(alpha, t), zero
        for i in range(n - 1, 0, -1):             # (P(X) - P(z)) / (X - z): q_(i-1) = c_i + z q_i
            carry = F.add(co[i], F.mul(z, carry))
            acc[i - 1] = F.add(acc[i - 1], F.mul(al, carry))
    a, b = get(da, 0), get(db, 0)
    return u64(w for i in range(n) for w in put(F.add(F.mul(a, acc[i]), F.mul(b, acc[i - 1]) if i else zero)))


def horner252(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P252
    return acc


def oods_252(cols_w, points, tcol, tpoint):
    fm = B252.from_mont
    C = {c: [fm(v) for v in M252.ints(cols_w[c])] for c in set(tcol)}
    zs, memo, out = [fm(v) for v in M252.ints(points)], {}, []
    for c, k in zip(tcol, tpoint):
        if (c, k) not in memo:
            memo[(c, k)] = B252.to_mont(horner252(C[c], zs[k]))
        out.append(memo[(c, k)])
    return M252.words(out) if out else np.zeros(0, dtype=np.uint64)


def ref_compose_252_division(n, cols_w, points, tcol, tpoint, alpha, da, db):
    """synthetic division of every term's polynomial by X - z, the alpha-weighted sum, the degree adjustment: Python integers"""
    p, fm = P252, B252.from_mont
    zs, al = [fm(v) for v in M252.ints(points)], [fm(v) for v in M252.ints(alpha)]
    a, b = fm(M252.ints(da)[0]), fm(M252.ints(db)[0])
    acc = [0] * n
    for t in range(len(tcol)):
        c = [fm(v) for v in M252.ints(cols_w[tcol[t]])]
        q, carry = [0] * n, 0
        for i in range(n - 1, 0, -1):             # (P(X) - P(z)) / (X - z): q_(i-1) = c_i + z q_i
            carry = (c[i] + zs[tpoint[t]] * carry) % p
            q[i - 1] = carry
        acc = [(s + al[t] * v) % p for s, v in zip(acc, q)]
    return M252.words([B252.to_mont((a * acc[i] + (b * acc[i - 1] if i else 0)) % p) for i in range(n)])


def check_compose_252_identity(log_n, got, cols_w, points, tcol, tpoint, alpha, ood, da, db):
    """out(x) = (a + b x) sum_t alpha_t (P_ct(x) - ood_t) / (x - z_pt) at the n points of the coset 5<w_n> (the call itself works on
    3<w_n>): n values of a polynomial with n coefficients, so every coefficient follows.  Evaluations by the C oracle's transform."""
    n, off = 1 << log_n, 5
    offw = M252.words([B252.to_mont(off)])
    lhs = M252.ints(cref.ntt252(got, log_n, False, offw))
    ev = {c: cref.ntt252(cols_w[c], log_n, False, offw) for c in set(tcol)}
    want = ref_rows_252([off * pow(B252.root_of_unity(n), i, P252) % P252 for i in range(n)], [ev.get(c, cols_w[c]) for c in range(len(cols_w))],
                        points, tcol, tpoint, alpha, ood, da, db)
    same(M252.words(lhs), want, "the evaluation identity on the coset 5<w_n>")


# ------------------------------------------------------------------------------------------------------------------
# references: ms_horner_eval
# ------------------------------------------------------------------------------------------------------------------
def ref_horner(cf, pf, n, cols_w, qcol, qpoints):
    pw = PW[pf]
    if n == 0 or not qcol:
        return np.zeros(len(qcol) * pw, dtype=np.uint64)
    if pf == F252:
        fm = B252.from_mont
        C = {c: [fm(v) for v in M252.ints(cols_w[c])] for c in set(qcol)}
        return M252.words([B252.to_mont(horner252(C[c], fm(z))) for c, z in zip(qcol, M252.ints(qpoints))])
    return np.concatenate([cref.horner_eval(cols_w[c], PW[cf], qpoints[q * pw:(q + 1) * pw]) for q, c in enumerate(qcol)])


def call_horner(pl, cf, pf, n, bufs, qcol, qpoints, out, ncols=None):
    qp = qpoints if qpoints.size else np.zeros(4, dtype=np.uint64)
    return pl.lib.ms_horner_eval(pl.handle, cf, pf, n, _table(bufs), len(bufs) if ncols is None else ncols, _uints(qcol), qp.ctypes.data, len(qcol),
                                 out.ctypes.data)


def check_horner(pl, cf, pf, n, cols_w, qcol, qpoints, want=None, what="horner"):
    pw = PW[pf]
    bufs = [Buf(pl, w) for w in cols_w]
    out = np.concatenate([np.full(len(qcol) * pw, SENTINEL, dtype=np.uint64), GUARD])
    rc = call_horner(pl, cf, pf, n, bufs, qcol, qpoints, out)
    assert rc == MS_OK, f"{what}: status {rc}: {pl.lib.ms_last_error().decode()}"
    assert np.array_equal(out[len(qcol) * pw:], GUARD), what + ": words behind the last result were written"
    same(out[:len(qcol) * pw], ref_horner(cf, pf, n, cols_w, qcol, qpoints) if want is None else want, what)
    for b, w in zip(bufs, cols_w):
        same(b.read(), w, what + ": a column after the call")


__all__ = [n for n in dir() if not n.startswith("_")] + ["GL_EDGE"]
