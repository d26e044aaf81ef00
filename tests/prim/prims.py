"""TEST INFRASTRUCTURE ONLY: the field primitives of ministark_amd/csrc one at a time (tests/test_field_primitives.py).

tests/prim/field_prims.hip is built twice -- by hipcc for gfx950 (the inline assembly, builtins and constant-address-space loads of
the device branches) and by g++ against the simulator of tests/emu (the #else branches) -- and both run the same inputs.  Inputs are
drawn per edge class: one class per branch or fix-up of a primitive, plus uniform inputs and edge values crossed pairwise.  Every
class asserts its defining condition on each input it keeps, so a generator bug cannot leave a class empty or off target.  Expected
values are Python integers computed from the contract in each primitive's header comment, never from either build; the pieces of
the RPO-256 permutation (family "rpo") are checked against oracle/pyref/rpo.py.

    python tests/prim/prims.py device LIB.so IN.npz OUT.npz    # every op of IN on one build, one process, stops at the first failure
"""
import ctypes
import hashlib
import os
import random
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "ministark_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
SRC = os.path.join(HERE, "field_prims.hip")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.pyref import rpo as pyrpo  # noqa: E402    (the reference of the rpo family)
OUT = os.path.join(EMU, "_build")                  # git-ignored
BLOCK = 64                                         # lanes per block in field_prims.hip: pool and twiddle slots are per block
FAMILIES = ["gl", "gld", "limb", "acc", "f252", "rpo"]


# ---- building ------------------------------------------------------------------------------------------------------------------
def _command(kind, so):
    if kind == "device":
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        from ministark_amd.build import HIPCC, FLAGS
        return [HIPCC] + FLAGS + ["-shared", "-I" + CSRC, SRC, "-o", so]
    return ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + EMU, "-I" + CSRC, "-Wall", "-Wno-unused-function",
            "-Wno-unknown-pragmas", "-DMS_NO_JIT", "-x", "c++", SRC, "-x", "none", os.path.join(EMU, "emu_runtime.cpp"), "-o", so]


def build(kind, timeout=900):
    """kind "device" (hipcc, gfx950) or "host" (g++ + the simulator) -> the shared object, rebuilt when a source changed."""
    so = os.path.join(OUT, "libfield_prims_%s.so" % ("hip" if kind == "device" else "emu"))
    cmd = _command(kind, so)
    h = hashlib.sha256(" ".join(cmd).replace(ROOT, "").encode())     # the same on any checkout path
    deps = [SRC, os.path.join(EMU, "emu_runtime.cpp"), os.path.join(EMU, "hip", "hip_runtime.h")]
    deps += sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h"))
    for p in deps:
        h.update(os.path.basename(p).encode())
        with open(p, "rb") as f:
            h.update(f.read())
    want, stamp = h.hexdigest(), so + ".srchash"
    if os.path.exists(so) and os.path.exists(stamp) and open(stamp).read().strip() == want:
        return so
    os.makedirs(OUT, exist_ok=True)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("building %s failed (%d):\n%s\n%s" % (so, r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-4000:]))
    with open(stamp, "w") as f:
        f.write(want + "\n")
    return so


class Lib:
    def __init__(self, so):
        self.dll = ctypes.CDLL(so)
        for fam in FAMILIES:
            fn = getattr(self.dll, "fp_" + fam)
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                           ctypes.c_void_p, ctypes.c_int]

    def run_raw(self, family, code, aux, inp, os_, tab):
        inp = np.ascontiguousarray(inp, dtype=np.uint64)
        tab = np.ascontiguousarray(tab, dtype=np.uint64)
        out = np.zeros((inp.shape[0], os_), dtype=np.uint64)
        rc = getattr(self.dll, "fp_" + family)(code, aux, inp.ctypes.data, inp.shape[1], out.ctypes.data, os_, inp.shape[0],
                                               tab.ctypes.data if tab.size else None, int(tab.size))
        if rc != 0:
            raise RuntimeError("fp_%s op %d: host entry returned %d" % (family, code, rc))
        return out

    def run(self, op):
        return self.run_raw(op.family, op.code, op.aux, op.inputs(), op.os, op.tab())


# ---- the fields -----------------------------------------------------------------------------------------------------------------
M24, M28, M32, M64 = (1 << 24) - 1, (1 << 28) - 1, (1 << 32) - 1, (1 << 64) - 1
P = (1 << 64) - (1 << 32) + 1                      # Goldilocks
EPS = M32                                          # 2^64 mod p
RINV = pow(1 << 64, -1, P)                         # Montgomery radix 2^64
Q96 = (1 << 96) + 1                                # the limb form is a representation mod 2^96 + 1 (p divides it)
W16 = pow(pow(7, (P - 1) >> 32, P), 1 << 28, P)    # arkworks' 16th root of unity: generator 7, two-adicity 32
W16I = pow(W16, -1, P)
assert W16 == P - (1 << 60)                        # gl_dev.h: w_16 = 2^156 = -2^60
BIAS = [(1 << 29) + 32, (1 << 29) - 32, (1 << 29) - 32, (1 << 29) - 32]
assert sum(b << (24 * k) for k, b in enumerate(BIAS)) == 32 * Q96      # gl_limb.h: the bias is 32 (2^96 + 1)
SWING = 2 ** 28.2                                  # gl_limb.h dft: "bias + a signed swing < 2^28.2 per limb"

P2 = (1 << 251) + 17 * (1 << 192) + 1              # the 252-bit StarkWare field
RINV2 = pow(1 << 256, -1, P2)

E64 = [0, 1, 2, EPS, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, 0xFFFFFFFE00000001, 0xFFFFFFFEFFFFFFFF, P - 2, P - 1, P, P + 1,
       M64 - 1, M64]
EC = [e for e in E64 if e < P]
E252 = [0, 1, 2, M64, 1 << 64, 1 << 128, (1 << 192) - 1, 1 << 192, (1 << 251) - 1, 1 << 251, (1 << 256) % P2, P2 - 2, P2 - 1]


def canon(r): return r.randrange(P)
def any64(r): return r.getrandbits(64)
def weak_hi(r): return P + r.randrange(M64 - P + 1)               # [p, 2^64)
def canon2(r): return r.randrange(P2)
def s32(x): x &= M32; return x - (1 << 32) if x >> 31 else x
def lval(ls): return sum(s32(l) << (24 * k) for k, l in enumerate(ls))
def w4(x): return [(x >> (64 * k)) & M64 for k in range(4)]
def unw4(ws): return sum(w << (64 * k) for k, w in enumerate(ws))
def digits9(x): return [(x >> (28 * k)) & M28 for k in range(8)] + [x >> 224]


def _hx(ws):
    return "[" + " ".join("%x" % w for w in ws) + "]"


def _eq(got, want):
    return None if list(got) == list(want) else "got %s want %s" % (_hx(got), _hx(want))


def _cong(got, want, mod=P):
    """a weak value: congruent to `want` (its 64-bit range is that of the word itself)"""
    return None if (got - want) % mod == 0 else "got %x, not congruent to %x" % (got, want % mod)


def _all(*msgs):
    for m in msgs:
        if m:
            return m
    return None


# ---- ops and their edge classes -----------------------------------------------------------------------------------------------
class Op:
    def __init__(self, family, name, code, is_, os_, check, aux=0):
        self.family, self.name, self.code, self.is_, self.os, self.check, self.aux = family, name, code, is_, os_, check, aux
        self.key = "%s.%s" % (family, name)
        self.rng = random.Random(self.key)
        self.rows, self.label, self.counts, self.table = [], [], {}, []

    def _keep(self, cname, row):
        assert len(row) <= self.is_, (self.key, cname, row)
        self.rows.append(list(row) + [0] * (self.is_ - len(row)))
        self.label.append(cname)
        self.counts[cname] = self.counts.get(cname, 0) + 1

    def add(self, cname, rows, cond=None):
        """fixed inputs; each must meet the class's condition"""
        for row in rows:
            assert cond is None or cond(row, len(self.rows)), "%s: class %s: %s does not meet its condition" % (self.key, cname, _hx(row))
            self._keep(cname, row)

    def gen(self, cname, count, make, cond=None, tries=4000):
        """`count` inputs make(rng, case index), each drawn again until the class's condition holds"""
        for _ in range(count):
            for _ in range(tries):
                row = make(self.rng, len(self.rows))
                if cond is None or cond(row, len(self.rows)):
                    break
            else:
                raise AssertionError("%s: class %s: no input meets its condition" % (self.key, cname))
            self._keep(cname, row)

    def inputs(self):
        return np.array(self.rows, dtype=np.uint64).reshape(len(self.rows), self.is_)

    def tab(self):
        return np.array(self.table, dtype=np.uint64)

    def summary(self):
        return "%s: %s" % (self.key, ", ".join("%s %d" % kv for kv in self.counts.items()))

    def verify(self, out, limit=3):
        bad = []
        for i, (a, o) in enumerate(zip(self.rows, out.tolist())):
            msg = self.check(a, o, i)
            if msg:
                bad.append("%s [%s] case %d in=%s: %s" % (self.key, self.label[i], i, _hx(a), msg))
                if len(bad) >= limit:
                    break
        return bad


def _pairs(xs, ys):
    return [[x, y] for x in xs for y in ys]


def _f2(f, g):
    return lambda r, i: [f(r), g(r)]


# gl.h: canonical add / sub / neg, weak add_lazy / sub_lazy, canon, reduce128, mul, the Montgomery forms, Fq3
def _r128(lo, hi):
    """reduce128's branches: (lo < hh, the r < t1 wrap, r before canon)"""
    hh, hl = hi >> 32, hi & M32
    t0 = (lo - hh) & M64
    if lo < hh:
        t0 = (t0 - EPS) & M64
    t1 = (hl << 32) - hl
    r = t0 + t1
    return lo < hh, r > M64, (r & M64) + (EPS if r > M64 else 0)


def _fq3_mul(a, b):                                # Fp[x] / (x^3 - 2)
    return [(a[0] * b[0] + 2 * (a[1] * b[2] + a[2] * b[1])) % P, (a[0] * b[1] + a[1] * b[0] + 2 * a[2] * b[2]) % P,
            (a[0] * b[2] + a[1] * b[1] + a[2] * b[0]) % P]


def _fq3_inv_check(a, o, i):
    if a[:3] == [0, 0, 0]:
        return _eq(o[:3], [0, 0, 0])
    if any(c >= P for c in o[:3]):
        return "not canonical: %s" % _hx(o[:3])
    x, y = [c * RINV % P for c in a[:3]], [c * RINV % P for c in o[:3]]
    return None if _fq3_mul(x, y) == [1, 0, 0] else "a * inv(a) != 1: inv = %s" % _hx(o[:3])


def _gl(n):
    ops = []

    def op(name, code, check):
        ops.append(Op("gl", name, code, 6, 3, check))
        return ops[-1]

    o = op("add", 0, lambda a, o, i: _eq(o[:1], [(a[0] + a[1]) % P]))
    o.add("edges", _pairs(EC, EC))
    o.gen("a+b>=p", n, _f2(canon, canon), lambda a, i: a[0] + a[1] >= P)
    o.gen("a+b<p", n, _f2(canon, canon), lambda a, i: a[0] + a[1] < P)
    o = op("sub", 1, lambda a, o, i: _eq(o[:1], [(a[0] - a[1]) % P]))
    o.add("edges", _pairs(EC, EC))
    o.gen("a<b", n, _f2(canon, canon), lambda a, i: a[0] < a[1])
    o.gen("a>=b", n, _f2(canon, canon), lambda a, i: a[0] >= a[1])
    o = op("neg", 2, lambda a, o, i: _eq(o[:1], [-a[0] % P]))
    o.add("edges", [[e] for e in EC])
    o.gen("uniform", n, lambda r, i: [canon(r)])
    o = op("add_lazy", 3, lambda a, o, i: _cong(o[0], a[0] + a[1]))
    o.add("edges", _pairs(E64, EC))
    o.gen("overflow", n, _f2(any64, canon), lambda a, i: a[0] + a[1] > M64)
    o.gen("a>=p", n, _f2(weak_hi, canon))
    o = op("sub_lazy", 4, lambda a, o, i: _cong(o[0], a[0] - a[1]))
    o.add("edges", _pairs(E64, EC))
    o.gen("borrow", n, _f2(any64, canon), lambda a, i: a[0] < a[1])
    o.gen("a>=p", n, _f2(weak_hi, canon))
    o = op("canon", 5, lambda a, o, i: _eq(o[:1], [a[0] % P]))
    o.add("edges", [[e] for e in E64])
    o.gen("[p,2^64)", n, lambda r, i: [weak_hi(r)])

    o = op("reduce128", 6, lambda a, o, i: _eq(o[:1], [(a[0] + (a[1] << 64)) % P]))
    o.add("edges", _pairs(E64, E64))
    o.gen("lo<hh", n, lambda r, i: [r.getrandbits(32), any64(r)], lambda a, i: _r128(*a[:2])[0])
    o.gen("r<t1 wrap", n, _f2(any64, any64), lambda a, i: _r128(*a[:2])[1])

    def pre_canon_high(r, i):                      # r = t0 + t1 lands in [p, 2^64) without a borrow or a wrap
        hl = r.getrandbits(32)
        t1 = (hl << 32) - hl
        z = weak_hi(r)
        hh = r.randrange(min(t1, M32) + 1)
        return [max(z - t1, 0) + hh, (hh << 32) | hl]
    o.gen("[p,2^64) before canon", n, pre_canon_high,
          lambda a, i: a[0] <= M64 and not any(_r128(*a[:2])[:2]) and _r128(*a[:2])[2] >= P)
    o.gen("uniform", n, _f2(any64, any64))

    o = op("mul", 7, lambda a, o, i: _eq(o[:1], [a[0] * a[1] % P]))
    o.add("edges", _pairs(E64, E64))
    o.gen("uniform", n, _f2(any64, any64))
    o = op("mont_mul", 8, lambda a, o, i: _eq(o[:1], [a[0] * a[1] * RINV % P]))
    o.add("edges", _pairs(EC, EC))
    o.gen("uniform", n, _f2(canon, canon))
    o = op("to_mont", 9, lambda a, o, i: _eq(o[:1], [(a[0] << 64) % P]))
    o.add("edges", [[e] for e in EC])
    o.gen("uniform", n, lambda r, i: [canon(r)])
    o = op("from_mont", 10, lambda a, o, i: _eq(o[:1], [a[0] * RINV % P]))
    o.add("edges", [[e] for e in EC])
    o.gen("uniform", n, lambda r, i: [canon(r)])
    o = op("mont_pow", 11, lambda a, o, i: _eq(o[:1], [(pow(a[0] * RINV % P, a[1], P) << 64) % P]))
    o.add("edges", _pairs(EC, [0, 1, 2, 3, P - 2, P - 1, M64]))
    o.gen("uniform", n, _f2(canon, any64))

    def mont_inv(a, o, i):
        x = a[0] * RINV % P
        return _eq(o[:1], [(pow(x, -1, P) << 64) % P if x else 0])
    o = op("mont_inv", 12, mont_inv)
    o.add("edges", [[e] for e in EC])
    o.gen("uniform", n, lambda r, i: [canon(r)])

    def fq3_mul(a, o, i):
        x, y = [c * RINV % P for c in a[:3]], [c * RINV % P for c in a[3:6]]
        return _eq(o[:3], [(c << 64) % P for c in _fq3_mul(x, y)])
    o = op("fq3_mont_mul", 13, fq3_mul)
    o.gen("edge components", n, lambda r, i: [r.choice(EC) for _ in range(6)])
    o.gen("uniform", n, lambda r, i: [canon(r) for _ in range(6)])
    o = op("fq3_mont_inv", 14, _fq3_inv_check)
    o.add("zero and units", [[0, 0, 0], [EPS, 0, 0], [0, EPS, 0], [0, 0, EPS], [P - 1, P - 1, P - 1]])
    o.gen("edge components", n, lambda r, i: [r.choice(EC) for _ in range(3)])
    o.gen("uniform", n, lambda r, i: [canon(r) for _ in range(3)])
    return ops


# gl_dev.h: mmul, the lazy add / sub, canon, mul_pow2, the butterflies and the radix-16 networks
def _pow2_branch(S, x):
    """mul_pow2<S>'s fix-up: S <= 32 the overflow of L + H EPS, S >= 64 the borrow of t - (y2 : y1)"""
    if S <= 32:
        return ((x >> (64 - S)) * EPS + ((x << S) & M64)) > M64
    rr = S - 64
    y0, y1, y2 = ((x & M32) << rr) & M32, (x >> (32 - rr)) & M32, (x >> 32) >> (32 - rr)
    return y0 * EPS < ((y2 << 32) | y1)


def _pow2_fixup(S):
    """inputs that reach the fix-up: S <= 32 L just below 2^64, S >= 64 a small y0"""
    if S <= 32:
        return lambda r, i: [(r.getrandbits(S) << (64 - S)) | ((1 << (64 - S)) - 1 - r.getrandbits(20))]
    rr = S - 64
    return lambda r, i: [((any64(r) >> (32 - rr)) << (32 - rr)) | r.getrandbits(4)]


def _dft_check(N, inv, NA=None):
    w = pow(W16I if inv else W16, 16 // N, P)
    na = N if NA is None else NA

    def check(a, o, i):
        for c in range(N):
            m = _cong(o[c], sum(a[k] * pow(w, k * c, P) for k in range(na)))
            if m:
                return "X[%d] %s" % (c, m)
        return None
    return check


def _gld(n):
    ops = []

    def op(name, code, check):
        ops.append(Op("gld", name, code, 16, 16, check))
        return ops[-1]

    o = op("mmul", 0, lambda a, o, i: _eq(o[:1], [a[0] * a[1] * RINV % P]))
    o.add("edges", _pairs(E64, EC))
    o.gen("a>=p", n, _f2(weak_hi, canon))
    o.gen("uniform", n, _f2(any64, canon))
    o = op("add_lazy", 1, lambda a, o, i: _cong(o[0], a[0] + a[1]))
    o.add("edges", _pairs(E64, EC))
    o.gen("overflow", n, _f2(any64, canon), lambda a, i: a[0] + a[1] > M64)
    o.gen("no overflow", n, _f2(any64, canon), lambda a, i: a[0] + a[1] <= M64)
    o = op("sub_lazy", 2, lambda a, o, i: _cong(o[0], a[0] - a[1]))
    o.add("edges", _pairs(E64, EC))
    o.gen("borrow", n, _f2(any64, canon), lambda a, i: a[0] < a[1])
    o.gen("no borrow", n, _f2(any64, canon), lambda a, i: a[0] >= a[1])
    o = op("canon", 3, lambda a, o, i: _eq(o[:1], [a[0] % P]))       # what hipcc (ROCm 7.2) once miscompiled
    o.add("edges", [[e] for e in E64])
    o.add("[p,2^64) ends", [[P], [P + 1], [M64 - 1], [M64]], lambda a, i: a[0] >= P)
    o.gen("[p,2^64)", n, lambda r, i: [weak_hi(r)])
    o.gen("uniform", n, lambda r, i: [any64(r)])
    for k, S in enumerate(range(12, 96, 12)):
        o = op("mul_pow2<%d>" % S, 10 + k, lambda a, o, i, S=S: _eq(o[:1], [(a[0] << S) % P]))
        o.add("edges", [[e] for e in E64])
        o.gen("[p,2^64)", n, lambda r, i: [weak_hi(r)])
        o.gen("uniform", n, lambda r, i: [any64(r)])
        if S <= 32 or S >= 64:
            o.gen("fix-up", n, _pow2_fixup(S), lambda a, i, S=S: _pow2_branch(S, a[0]))
            o.gen("no fix-up", n, lambda r, i: [any64(r)], lambda a, i, S=S: not _pow2_branch(S, a[0]))
    for inv in (0, 1):
        for E in range(8):
            for vc in (0, 1):
                w = pow(W16I if inv else W16, E, P)

                def check(a, o, i, w=w):
                    return _all(_cong(o[0], a[0] + w * a[1]), _cong(o[1], a[0] - w * a[1]))
                o = op("bfly<%d,%d,%d>" % (inv, E, vc), 100 + 16 * inv + 2 * E + vc, check)
                vgen = canon if vc else any64
                o.add("edges", _pairs(E64, EC if vc else E64))
                o.gen("u>=p", n, _f2(weak_hi, vgen))
                if not vc:
                    o.gen("v>=p", n, _f2(any64, weak_hi))
                o.gen("uniform", n, _f2(any64, vgen))
    for N in (2, 4, 8, 16):
        for inv in (0, 1):
            o = op("dft_lazy<%d,%d>" % (N, inv), 200 + 2 * N + inv, _dft_check(N, inv))
            o.add("all p-1", [[P - 1] * N])
            o.gen("edges", n, lambda r, i, N=N: [r.choice(EC) for _ in range(N)])
            o.gen("uniform", n, lambda r, i, N=N: [canon(r) for _ in range(N)])
    for NA in (1, 2, 4):
        for inv in (0, 1):
            o = op("dft16_pruned<%d,%d>" % (NA, inv), 300 + 2 * NA + inv, _dft_check(16, inv, NA))
            o.add("all p-1", [[P - 1] * NA])
            o.gen("edges", n, lambda r, i, NA=NA: [r.choice(EC) for _ in range(NA)])
            o.gen("uniform", n, lambda r, i, NA=NA: [canon(r) for _ in range(NA)])
    return ops


# gl_limb.h: limbs travel as 32-bit two's-complement words
def _fold_t_sim(lo, hi):
    """fold_t's z = (m : a0) + t EPS before its fix-ups -> (wrapped, z mod 2^64)"""
    a0, a1, b0, b1 = lo & M32, lo >> 32, hi & M32, hi >> 32
    m = a1 + b0
    t = (b1 + (m >> 32)) & M32
    z = t * EPS + (((m & M32) << 32) | a0)
    return z > M64, z & M64


def _fold_h_wraps(a0, H):
    return (H >> 32) * EPS + (((H & M32) << 32) | (a0 & M32)) > M64


def _limb(n):
    ops = []

    def op(name, code, is_, os_, check):
        ops.append(Op("limb", name, code, is_, os_, check))
        return ops[-1]

    def from_u64(a, o, i):
        if not (o[0] <= M24 and o[1] <= M24 and o[2] < 1 << 16 and o[3] == 0):
            return "limb out of range: %s" % _hx(o[:4])
        return None if o[0] + (o[1] << 24) + (o[2] << 48) == a[0] else "limbs %s do not make %x" % (_hx(o[:4]), a[0])
    o = op("from_u64", 0, 1, 4, from_u64)
    o.add("edges", [[e] for e in E64])
    o.gen("uniform", n, lambda r, i: [any64(r)])

    def perm(a, o, i):
        v = (a[0] << 32) | a[1]
        return _eq(o[:2], [(v >> 24) & M24, (v >> 16) & M24])
    o = op("perm", 1, 2, 2, perm)
    e32 = [0, 1, 0xFF, 0xFF00, 0x00FFFFFF, 0xFF000000, 0x80000000, 0x12345678, M32]
    o.add("edges", _pairs(e32, e32))
    o.gen("uniform", n, lambda r, i: [r.getrandbits(32), r.getrandbits(32)])

    def mul_to_limbs(a, o, i):
        if any(abs(s32(l)) >= 1 << 24 for l in o[:4]):
            return "|limb| >= 2^24: %s" % _hx(o[:4])
        return _cong(lval(o[:4]), a[0] * a[1], Q96)
    o = op("mul_to_limbs", 2, 2, 4, mul_to_limbs)
    o.add("edges", _pairs(E64, E64))
    o.gen("uniform", n, _f2(any64, any64))

    def half_shift(a, o, i):
        bound = (1 << 24) - (-max(abs(s32(l)) for l in a[:4]) // (1 << 12))
        if any(abs(s32(l)) > bound for l in o[:4]):
            return "limb above 2^24 + max|x| / 2^12: %s" % _hx(o[:4])
        return _cong(lval(o[:4]), lval(a[:4]) << 12, Q96)
    o = op("half_shift", 3, 4, 4, half_shift)
    i32e = [-(1 << 31), -(1 << 24), -4096, -1, 0, 1, 4095, (1 << 24) - 1, (1 << 31) - 1]
    o.gen("negative", n, lambda r, i: [r.randrange(1 << 31, 1 << 32) for _ in range(4)], lambda a, i: all(s32(l) < 0 for l in a))
    o.gen("edges", n, lambda r, i: [r.choice(i32e) & M32 for _ in range(4)])
    o.gen("uniform", n, lambda r, i: [r.getrandbits(32) for _ in range(4)])

    # butterflies: limbs up to 2^30 in magnitude (a biased network value plus its swing), so that u +- t stays inside 32 bits
    lim = (1 << 30) - 1
    for k in range(16):
        S = 12 * k

        def bfly(a, o, i, S=S):
            u, t = lval(a[:4]), lval(a[4:8]) << S
            return _all(_cong(lval(o[:4]), u + t, Q96), _cong(lval(o[4:8]), u - t, Q96))
        o = op("bfly<%d>" % S, 100 + k, 8, 8, bfly)
        o.gen("max magnitude", n, lambda r, i: [r.choice((lim, -lim)) & M32 for _ in range(8)])
        o.gen("nonnegative", n, lambda r, i: [r.randrange(1 << 30) for _ in range(8)])
        o.gen("uniform", n, lambda r, i: [r.randrange(-lim, lim + 1) & M32 for _ in range(8)])

    def net_check(N, inv, bias, NA=None):
        w = pow(W16I if inv else W16, 16 // N, P)
        na = N if NA is None else NA

        def check(a, o, i):
            x = [lval(a[4 * k:4 * k + 4]) for k in range(na)]
            for c in range(N):
                ls = o[4 * c:4 * c + 4]
                for k in range(4):
                    d = s32(ls[k]) - (BIAS[k] if bias else 0)
                    if abs(d) >= SWING:
                        return "X[%d] limb %d: swing %d >= 2^28.2" % (c, k, d)
                    if bias and not 0 <= s32(ls[k]) < 1 << 30:
                        return "X[%d] limb %d = %d outside mul_fold's [0, 2^30)" % (c, k, s32(ls[k]))
                m = _cong(lval(ls), sum(x[k] * pow(w, k * c, P) for k in range(na)))
                if m:
                    return "X[%d] %s" % (c, m)
            return None
        return check

    mx = (1 << 24) - 1                             # the stated input bound |l_i| < 2^24
    net_classes = [("all +max", lambda r, m: [mx] * m), ("all -max", lambda r, m: [-mx & M32] * m),
                   ("max, random signs", lambda r, m: [r.choice((mx, -mx)) & M32 for _ in range(m)]),
                   ("uniform", lambda r, m: [r.randrange(-mx, mx + 1) & M32 for _ in range(m)])]
    for N in (2, 4, 8, 16):
        for inv in (0, 1):
            for bias in (0, 1):
                o = op("dft<%d,%d,%d>" % (N, inv, bias), 200 + 4 * N + 2 * inv + bias, 4 * N, 4 * N, net_check(N, inv, bias))
                for cname, g in net_classes:
                    o.gen(cname, n, lambda r, i, g=g, N=N: g(r, 4 * N))
    for NA in (1, 2, 4):
        for inv in (0, 1):
            o = op("dft16_pruned<%d,%d>" % (NA, inv), 300 + 2 * NA + inv, 4 * NA, 64, net_check(16, inv, 1, NA))
            for cname, g in net_classes:
                o.gen(cname, n, lambda r, i, g=g, NA=NA: g(r, 4 * NA))

    # fold_t: (acc_lo, acc_hi) with acc_lo + acc_hi 2^32 < 2^96
    def below96(a, i):
        return a[0] + (a[1] << 32) < 1 << 96

    def z_high(r, i):                              # z in [p, 2^64) without a wrap
        z = weak_hi(r)
        t = r.randrange(min(z // EPS, M32) + 1)
        base = z - t * EPS
        m, a0 = base >> 32, base & M32
        b0 = r.randrange(m + 1)
        return [((m - b0) << 32) | a0, (t << 32) | b0]

    def near96(r, i):                              # acc_hi = 2^64 - k: its top word is all ones
        k = r.randrange(1, 256)
        return [r.randrange(max(0, (k << 32) - (1 << 36)), k << 32), (1 << 64) - k]
    for canon_ in (0, 1):
        o = op("fold_t<%d>" % canon_, 400 + canon_, 2, 1,
               lambda a, o, i, c=canon_: _eq(o[:1], [(a[0] + (a[1] << 32)) % P]) if c else _cong(o[0], a[0] + (a[1] << 32)))
        o.gen("acc just below 2^96", n, near96, lambda a, i: (1 << 96) - (1 << 40) <= a[0] + (a[1] << 32) < 1 << 96)
        o.gen("z wraps", n, _f2(any64, any64), lambda a, i: below96(a, i) and _fold_t_sim(*a[:2])[0])
        o.gen("z in [p,2^64)", n, z_high, lambda a, i: below96(a, i) and not _fold_t_sim(*a[:2])[0] and _fold_t_sim(*a[:2])[1] >= P)
        o.gen("uniform", n, _f2(any64, any64), below96)

    o = op("fold_h", 402, 2, 1, lambda a, o, i: _cong(o[0], (a[0] & M32) + (a[1] << 32)))
    o.add("edges", _pairs([0, 1, M32], [0, 1, M32, M32 << 32, P - 1, 1 << 63, M64]))
    o.gen("h1 EPS + base >= 2^64", n, lambda r, i: [r.getrandbits(32), any64(r)], lambda a, i: _fold_h_wraps(a[0], a[1]))
    o.gen("h1 EPS + base < 2^64", n, lambda r, i: [r.getrandbits(32), any64(r)], lambda a, i: not _fold_h_wraps(a[0], a[1]))

    # mul_fold / mul_fold_co: limbs in [0, 2^30); four copies of a twiddle per table slot (slot = block mod slots), any
    # representatives below 2^64 -- canonical, canonical + p where that fits, hi words all ones, all ones
    nslot = 16

    def twiddle_table(r):
        tab = []
        for s in range(nslot):
            w = canon(r)
            ws = [(w << (24 * k)) % P for k in range(4)]
            if s % 4 == 1:
                ws = [x + P if x + P <= M64 else x for x in ws]
            elif s % 4 == 2:
                ws = [(M32 << 32) | r.getrandbits(32) for _ in range(4)]
            elif s % 4 == 3:
                ws = [M64] * 4
            tab += ws
        return tab

    def copies(op_, i):
        s = (i // BLOCK) % nslot
        return op_.table[4 * s:4 * s + 4]

    lmax = (1 << 30) - 1
    limb_gens = [("limb edges", lambda r, i: [r.choice((0, 1, 1 << 29, lmax)) for _ in range(4)]),
                 ("all 2^30-1", lambda r, i: [lmax] * 4),
                 ("uniform", lambda r, i: [r.randrange(1 << 30) for _ in range(4)])]
    for code, co, canon_ in ((410, 0, 0), (411, 0, 1), (412, 1, 0), (413, 1, 1)):
        o = op("%s<%d>" % ("mul_fold_co" if co else "mul_fold", canon_), code, 4, 1, None)
        o.table = twiddle_table(o.rng)

        def check(a, o_, i, op_=o, canon_=canon_):
            want = sum(l * w for l, w in zip(a[:4], copies(op_, i)))
            return _eq(o_[:1], [want % P]) if canon_ else _cong(o_[0], want)
        o.check = check

        def wraps(a, i, op_=o, co=co):
            W = copies(op_, i)
            alo = sum(l * (w & M32) for l, w in zip(a[:4], W))
            ahi = sum(l * (w >> 32) for l, w in zip(a[:4], W))
            return _fold_h_wraps(alo, ahi + (alo >> 32)) if co else _fold_t_sim(alo, ahi)[0]
        for cname, g in limb_gens:
            o.gen(cname, n, g)
        o.gen("fold wraps 2^64", n, lambda r, i: [r.randrange(1 << 28, 1 << 30) for _ in range(4)], wraps)
        # (against copies whose hi words are all ones the fold wraps for every limb sum above 1)
        o.gen("fold stays below 2^64", n, lambda r, i: [r.randrange(1 << r.randrange(1, 31)) if r.getrandbits(1) else 0 for _ in range(4)],
              lambda a, i, w=wraps: not w(a, i))

    o = op("w4x4_at+mul_fold_co", 414, 4, 4, None)
    o.table = twiddle_table(o.rng)

    def check414(a, o_, i, op_=o):
        s4 = 4 * ((i // BLOCK) % (nslot // 4))
        for k in range(4):
            W = op_.table[4 * (s4 + k):4 * (s4 + k) + 4]
            m = _cong(o_[k], sum(l * w for l, w in zip(a[:4], W)))
            if m:
                return "copy %d: %s" % (k, m)
        return None
    o.check = check414
    for cname, g in limb_gens:
        o.gen(cname, n, g)

    def mul3(a, o, i):
        x = a[0]
        want = (x & M24) * a[1] + ((x >> 24) & M24) * a[2] + (x >> 48) * a[3]
        if not (o[0] <= M24 and o[1] <= M24 and o[2] <= M24 and o[3] < 1 << 18):
            return "limb out of range: %s" % _hx(o[:4])
        return None if lval(o[:4]) == want else "limbs %s do not make %x" % (_hx(o[:4]), want)
    o = op("mul3_to_limbs", 420, 4, 4, mul3)
    o.add("edges, all-ones copies", [[e, M64, M64, M64] for e in E64])
    o.gen("edges", n, lambda r, i: [r.choice(E64) for _ in range(4)])
    o.gen("uniform", n, lambda r, i: [any64(r) for _ in range(4)])

    for code, name, canon_ in ((430, "to_weak<0>", 0), (431, "to_weak<1>", 1), (432, "to_canon", 1)):
        def to_weak(a, o, i, canon_=canon_):
            v = sum(l << (24 * k) for k, l in enumerate(a[:4]))
            return _eq(o[:1], [v % P]) if canon_ else _cong(o[0], v)
        o = op(name, code, 4, 1, to_weak)
        for cname, g in limb_gens:
            o.gen(cname, n, g)
    return ops


# eval_kernels.h: Acc6 (Goldilocks), AccQ (Fq3), Acc19 (252-bit) and f252::reduce_columns
def _split22(c):
    return c & 0x3FFFFF, (c >> 22) & 0x3FFFFF, c >> 44


def _acc6(pairs):
    """the six columns of acc_mac_limbs over (v, c) pairs: v cut at 32 bits, c into 22 / 22 / 20-bit limbs"""
    S = [0] * 6
    for v, c in pairs:
        y = _split22(c)
        for j in range(3):
            S[j] += (v & M32) * y[j]
            S[3 + j] += (v >> 32) * y[j]
    return S


def _acc6_top_carry(pairs):
    """acc_reduce's `sum < top` carry: the low columns plus the top column's low 52 bits reach 2^128"""
    S = _acc6(pairs)
    low = S[0] + (S[1] << 22) + (S[2] << 44) + (S[3] << 32) + (S[4] << 54)
    return low + ((S[5] & ((1 << 52) - 1)) << 76) >= 1 << 128


def _check_acc6(pairs, raw, red):
    S = _acc6(pairs)
    if any(s > M64 for s in S):
        return "a column exceeds 64 bits: the term limit does not hold"
    total = sum(v * c for v, c in pairs)
    assert S[0] + (S[1] << 22) + (S[2] << 44) + (S[3] << 32) + (S[4] << 54) + (S[5] << 76) == total
    return _all(_eq(raw, S), _eq([red], [total * RINV % P]))


def _pack22(c):
    y0, y1, y2 = _split22(c)
    return [y0 | (y1 << 32), y2]


def _pack9(c):
    d = digits9(c)
    return [d[0] | (d[1] << 32), d[2] | (d[3] << 32), d[4] | (d[5] << 32), d[6] | (d[7] << 32), d[8]]


def _acc19(pairs):
    c = [0] * 19
    for v, b in pairs:
        x, y = digits9(v), digits9(b)
        for i in range(9):
            for j in range(9):
                c[i + j] += x[i] * y[j]
    return c


def _check_cols(c, raw, red_words, canon_=True):
    if any(x > M64 for x in c):
        return "a column exceeds 64 bits: the product limit does not hold"
    V = sum(x << (28 * k) for k, x in enumerate(c))
    red = unw4(red_words)
    m = _eq(raw, c) if raw is not None else None
    if canon_:
        return _all(m, None if red == V * RINV2 % P2 else "reduced %x want %x" % (red, V * RINV2 % P2))
    return _all(m, ("reduced %x >= 2p" % red) if red >= 2 * P2 else None, _cong(red, V * RINV2, P2))


def _acc(n):
    ops = []
    big = max(2, n // 16)                          # cases per class at 255 and more terms

    def op(name, code, is_, aux):
        ops.append(Op("acc", name, code, is_, {0: 7, 1: 7, 10: 23, 11: 23, 12: 4, 13: 4}.get(code, 21), None, aux))
        return ops[-1]

    hi20 = 0xFFFFF << 44                           # canonical words whose top limb y2 is all ones

    def near_max(r):
        return r.choice((P - 1, 0xFFFFFFFEFFFFFFFF, hi20 + r.randrange(P - hi20)))

    def pool(op_, K=17):
        """Goldilocks constant pool: the two largest canonical words and words with y2 all ones"""
        op_.consts = [P - 1, 0xFFFFFFFEFFFFFFFF] + [hi20 + op_.rng.randrange(P - hi20) for _ in range(K - 2)]
        op_.table = [w for c in op_.consts for w in _pack22(c)]

    def const(op_, i, t):
        return op_.consts[(i // BLOCK + t) % len(op_.consts)]

    # Acc6.  The largest operands the evaluator admits are canonical words (its registers and its constants are canonical
    # Montgomery words): p - 1 has the largest high half, 2^64 - 2^32 - 1 the largest low half with all limbs near full.
    for T in (1, 2, 511, 512):
        for code in (0, 1):
            o = op("%s[T=%d]" % ("acc_macp" if code == 0 else "acc_macc", T), code, 2 * T if code == 0 else T, T)
            if code == 1:
                pool(o)

            def pairs(a, i, o=o, T=T, code=code):
                if code == 0:
                    return [(a[2 * t], a[2 * t + 1]) for t in range(T)]
                return [(a[t], const(o, i, t)) for t in range(T)]
            o.check = lambda a, o_, i, pairs=pairs: _check_acc6(pairs(a, i), o_[:6], o_[6])
            cnt, per = (n if T <= 2 else big), (2 if code == 0 else 1)
            o.gen("all p-1", cnt, lambda r, i, T=T, per=per: [P - 1] * (per * T))
            o.gen("all 2^64-2^32-1", cnt, lambda r, i, T=T, per=per: [0xFFFFFFFEFFFFFFFF] * (per * T))
            o.gen("near max", cnt, lambda r, i, T=T, per=per: [near_max(r) for _ in range(per * T)])
            o.gen("uniform", cnt, lambda r, i, T=T, per=per: [canon(r) for _ in range(per * T)])
            if T >= 511:
                def carry_case(r, i, T=T, code=code, pairs=pairs):
                    # near-max terms, then the high half of the last v chosen so that the top column's low 52 bits land just
                    # below 2^52 (every constant here has y2 = 2^20 - 1): the 128-bit sum in acc_reduce then wraps
                    row = [near_max(r) for _ in range((2 if code == 0 else 1) * T)]
                    vi = 2 * (T - 1) if code == 0 else T - 1
                    if code == 0:
                        row[vi + 1] = hi20 + r.randrange(P - hi20)
                    row[vi] = 0
                    s5 = _acc6(pairs(row, i))[5]
                    y2 = pairs(row, i)[T - 1][1] >> 44
                    c1 = -(-(((1 << 52) - (1 << 38) - s5) % (1 << 52)) // y2)
                    row[vi] = (min(c1, M32 - 1) << 32) | r.getrandbits(32)
                    return row
                o.gen("sum < top carry", cnt, carry_case, lambda a, i, pairs=pairs: _acc6_top_carry(pairs(a, i)))

    # AccQ: ACC_MAX_TERMS_Q terms of each of the six forms
    for T in (1, 256):
        for code, name, per in ((2, "accq_macc_p_cp", 1), (3, "accq_macc_q_cp", 3), (4, "accq_macc_p_cq", 1), (5, "accq_macc_q_cq", 3),
                                (6, "accq_macp_p_p", 2), (7, "accq_macp_q_p", 4)):
            o = op("%s[T=%d]" % (name, T), code, per * T, T)
            if code in (2, 3):
                pool(o)
            elif code in (4, 5):                   # Fq3 constants: C0, C1, C2, 2 C1, 2 C2 (eval_regroup.h)
                o.consts = [[P - 1] * 3, [0xFFFFFFFEFFFFFFFF] * 3] + [[hi20 + o.rng.randrange(P - hi20) for _ in range(3)] for _ in range(9)]
                o.table = [w for c in o.consts for x in (c[0], c[1], c[2], 2 * c[1] % P, 2 * c[2] % P) for w in _pack22(x)]

            def comps(a, i, o=o, T=T, code=code):
                cs = [[], [], []]
                for t in range(T):
                    if code == 2:
                        cs[0].append((a[t], const(o, i, t)))
                    elif code == 3:
                        for k in range(3):
                            cs[k].append((a[3 * t + k], const(o, i, t)))
                    elif code in (4, 5):
                        C = const(o, i, t)
                        D1, D2 = 2 * C[1] % P, 2 * C[2] % P
                        if code == 4:
                            for k in range(3):
                                cs[k].append((a[t], C[k]))
                        else:
                            t0, t1, t2 = a[3 * t:3 * t + 3]
                            cs[0] += [(t0, C[0]), (t1, D2), (t2, D1)]
                            cs[1] += [(t0, C[1]), (t1, C[0]), (t2, D2)]
                            cs[2] += [(t0, C[2]), (t1, C[1]), (t2, C[0])]
                    elif code == 6:
                        cs[0].append((a[2 * t], a[2 * t + 1]))
                    else:
                        for k in range(3):
                            cs[k].append((a[4 * t + k], a[4 * t + 3]))
                return cs

            def check(a, o_, i, comps=comps):
                cs = comps(a, i)
                for k in range(3):
                    m = _check_acc6(cs[k], o_[6 * k:6 * k + 6], o_[18 + k])
                    if m:
                        return "component %d: %s" % (k, m)
                return None
            o.check = check
            cnt = n if T == 1 else big
            o.gen("all p-1", cnt, lambda r, i, T=T, per=per: [P - 1] * (per * T))
            o.gen("near max", cnt, lambda r, i, T=T, per=per: [near_max(r) for _ in range(per * T)])
            o.gen("uniform", cnt, lambda r, i, T=T, per=per: [canon(r) for _ in range(per * T)])

    # Acc19: ACC_MAX_TERMS_252 = 16 products of the largest canonical operands (2^251 - 1 has every digit full but the top one)
    full = (1 << 251) - 1
    for T in (1, 16):
        for code in (10, 11):
            o = op("%s[T=%d]" % ("acc19_macp" if code == 10 else "acc19_macc", T), code, 8 * T if code == 10 else 4 * T, T)
            if code == 11:
                o.consts = [full, P2 - 1] + [P2 - 1 - o.rng.getrandbits(200) for _ in range(5)]
                o.table = [w for c in o.consts for w in _pack9(c)]

            def pairs(a, i, o=o, T=T, code=code):
                if code == 10:
                    return [(unw4(a[8 * t:8 * t + 4]), unw4(a[8 * t + 4:8 * t + 8])) for t in range(T)]
                return [(unw4(a[4 * t:4 * t + 4]), const(o, i, t)) for t in range(T)]
            o.check = lambda a, o_, i, pairs=pairs: _check_cols(_acc19(pairs(a, i)), o_[:19], o_[19:23])
            per = 2 if code == 10 else 1
            o.gen("all 2^251-1", n, lambda r, i, T=T, per=per: w4(full) * (per * T))
            o.gen("all p-1", n, lambda r, i, T=T, per=per: w4(P2 - 1) * (per * T))
            o.gen("near p", n, lambda r, i, T=T, per=per: [w for _ in range(per * T) for w in w4(P2 - 1 - r.getrandbits(200))])
            o.gen("uniform", n, lambda r, i, T=T, per=per: [w for _ in range(per * T) for w in w4(canon2(r))])

    # reduce_columns on hand-built columns.  fp252.h: "with K canonical products in the columns the value is below (K / 31.9 + 1) p:
    # one conditional subtraction makes it canonical for K <= 30".  mac81 cannot build K = 30 (16 products per column), so the
    # columns are cut from V directly, with weight moved down from each column into the one below it (columns up to ~2^60).
    def columns(V, r):
        c = [(V >> (28 * k)) & M28 for k in range(18)] + [V >> (28 * 18)]
        for k in range(17, -1, -1):
            mv = r.randrange(min(c[k + 1], 1 << 32) + 1)
            c[k + 1] -= mv
            c[k] += mv << 28
        return c
    bound30 = 30 * (P2 - 1) ** 2
    for code, canon_ in ((12, True), (13, False)):
        o = op("reduce_columns<%d>" % canon_, code, 19, 0)
        o.check = lambda a, o_, i, canon_=canon_: _check_cols(a[:19], None, o_[:4], canon_)
        o.gen("just below 30 (p-1)^2", n, lambda r, i: columns(bound30 - r.getrandbits(200), r),
              lambda a, i: bound30 - (1 << 200) <= sum(x << (28 * k) for k, x in enumerate(a)) <= bound30)
        o.gen("16 products of 2^251-1", n, lambda r, i: _acc19([(full, full)] * 16))
        o.gen("uniform below 30 p^2", n, lambda r, i: columns(r.randrange(bound30), r))
    return ops


# fp252.h
def _f252(n):
    ops = []

    def op(name, code, check):
        ops.append(Op("f252", name, code, 8, 9, check))
        return ops[-1]

    def A(a): return unw4(a[:4])
    def B(a): return unw4(a[4:8])
    def row(x, y=0): return w4(x) + w4(y)
    edges = [row(x, y) for x in E252 for y in E252]

    o = op("add", 0, lambda a, o, i: _eq(o[:4], w4((A(a) + B(a)) % P2)))
    o.add("edges", edges)
    o.gen("a+b>=p", n, lambda r, i: row(canon2(r), canon2(r)), lambda a, i: A(a) + B(a) >= P2)
    o.gen("uniform", n, lambda r, i: row(canon2(r), canon2(r)))
    o = op("neg", 1, lambda a, o, i: _eq(o[:4], w4(-A(a) % P2)))
    o.add("edges", [row(x) for x in E252])
    o.gen("uniform", n, lambda r, i: row(canon2(r)))
    o = op("sub", 2, lambda a, o, i: _eq(o[:4], w4((A(a) - B(a)) % P2)))
    o.add("edges", edges)
    o.gen("a<b", n, lambda r, i: row(canon2(r), canon2(r)), lambda a, i: A(a) < B(a))
    o.gen("uniform", n, lambda r, i: row(canon2(r), canon2(r)))
    o = op("mul", 3, lambda a, o, i: _eq(o[:4], w4(A(a) * B(a) * RINV2 % P2)))
    o.add("edges", edges)
    o.gen("uniform", n, lambda r, i: row(canon2(r), canon2(r)))
    o = op("sqr", 4, lambda a, o, i: _eq(o[:4], w4(A(a) * A(a) * RINV2 % P2)))
    o.add("edges", [row(x) for x in E252])
    o.gen("uniform", n, lambda r, i: row(canon2(r)))
    o = op("inv", 5, lambda a, o, i: _eq(o[:4], w4((pow(A(a), -1, P2) << 512) % P2 if A(a) else 0)))
    o.add("edges", [row(x) for x in E252])
    o.gen("uniform", n, lambda r, i: row(canon2(r)))
    o = op("to_mont", 6, lambda a, o, i: _eq(o[:4], w4((A(a) << 256) % P2)))
    o.add("edges", [row(x) for x in E252])
    o.gen("uniform", n, lambda r, i: row(canon2(r)))
    o = op("from_mont", 7, lambda a, o, i: _eq(o[:4], w4(A(a) * RINV2 % P2)))
    o.add("edges", [row(x) for x in E252])
    o.gen("uniform", n, lambda r, i: row(canon2(r)))

    # mul_t<false>: any a < 2^256 with a canonical b -> below 2p, congruent to a b R^-1
    def mul_t(a, o, i):
        v = unw4(o[:4])
        return ("%x >= 2p" % v) if v >= 2 * P2 else _cong(v, A(a) * B(a) * RINV2, P2)
    o = op("mul_t<false>", 8, mul_t)
    o.add("a = 2^256-1", [row((1 << 256) - 1, y) for y in E252])
    o.gen("a in [p,2^256)", n, lambda r, i: row(r.getrandbits(256), canon2(r)), lambda a, i: A(a) >= P2)
    o.gen("uniform", n, lambda r, i: row(r.getrandbits(256), canon2(r)))

    def at_bound(r, i):
        x = r.getrandbits(256)
        return row(x, max((1 << 256) - 1 - x - r.randrange(4), 0))
    o = op("add_lazy", 9, lambda a, o, i: _eq(o[:4], w4(A(a) + B(a))))
    o.gen("a+b at 2^256-1", n, at_bound, lambda a, i: (1 << 256) - 4 <= A(a) + B(a) < 1 << 256)
    o.gen("uniform", n, lambda r, i: row(r.getrandbits(255), r.getrandbits(255)))
    for K, code in ((2, 10), (4, 11)):
        o = op("kp_minus<%d>" % K, code, lambda a, o, i, K=K: _eq(o[:4], w4(K * P2 - A(a))))
        o.add("ends", [row(0), row(1), row(P2), row(K * P2 - 1)])
        o.gen("near Kp", n, lambda r, i, K=K: row(K * P2 - 1 - r.getrandbits(64)))
        o.gen("uniform", n, lambda r, i, K=K: row(r.randrange(K * P2)))

    # reduce_lazy: q = floor(x / 2^251) is floor(x / p) or one more
    o = op("reduce_lazy", 12, lambda a, o, i: _eq(o[:4], w4(A(a) % P2)))
    o.add("around k p", [row(k * P2 + d) for k in range(32) for d in range(-3, 4) if 0 <= k * P2 + d < 1 << 256])
    o.add("around k 2^251", [row((k << 251) + d) for k in range(33) for d in range(-3, 4) if 0 <= (k << 251) + d < 1 << 256])
    o.add("top", [row((1 << 256) - 1), row((1 << 256) - 2)])
    o.gen("quotient one too large", n, lambda r, i: row(r.randrange(1, 32) * P2 - 1 - r.getrandbits(r.choice((8, 64, 190)))),
          lambda a, i: (A(a) >> 251) * P2 > A(a))
    o.gen("uniform", n, lambda r, i: row(r.getrandbits(256)))
    o = op("digits9", 13, lambda a, o, i: _eq(o[:9], digits9(A(a))))
    o.add("edges", [row(x) for x in E252 + [(1 << 256) - 1]])
    o.gen("uniform", n, lambda r, i: row(r.getrandbits(256)))
    return ops


# rpo_kernels.h, rpo_coin_kernels.h: the pieces of the RPO-256 permutation and the permutation in every device form.  The reference
# is oracle/pyref/rpo.py (Python integers on canonical values, pinned to external vectors by tests/test_rpo_parity.py); the device
# holds Montgomery words w = x 2^64 mod p, so a word goes through _val on its way in and through _word on its way out.  The MDS
# accumulator sees the words themselves: its classes are conditions on the integer sum of words.
E8 = [0, 1, P - 1, P - 2, M32, 1 << 32, (1 << 32) + 1, P - (1 << 32)]
assert all(e < P for e in E8)
UNITY_ORDERS = [2, 3, 4, 5, 8, 15, 16, 17, 257, 65537, 1 << 32]
assert all((P - 1) % d == 0 for d in UNITY_ORDERS)
# x^7 = 1 has no solution but x = 1: 7 does not divide p - 1, which is what makes x^7 a permutation.  In place of that (empty) class
# the S-boxes get elements of small order, whose squaring chains run through 1 and p - 1.
assert (P - 1) % 7 != 0


def _val(w): return w * RINV % P
def _word(x): return (x << 64) % P
def _vals(ws): return [_val(w) for w in ws]
def _words(xs): return [_word(x) for x in xs]
def _mds_sums(ws): return [sum(pyrpo.MDS_ROW[(k - m) % 12] * ws[k] for k in range(12)) for m in range(12)]
def _state(r): return [canon(r) for _ in range(12)]
def _edge_state(r): return [r.choice(E8) for _ in range(12)]


def _tag(name, msg):
    return "%s: %s" % (name, msg) if msg else None


def _rpo(n):
    ops = []
    n1, nm, np_ = 16 * n, 4 * n, max(2, n // 2)    # cases per class: one-element ops, MDS ops, whole permutations

    def op(name, code, is_, os_, check, aux=0):
        ops.append(Op("rpo", name, code, is_, os_, check, aux))
        return ops[-1]

    # ---- the MDS layer: sum_k MDS[m][k] s[k] as one integer below 160 2^64, reduced once
    def mds_want(a):
        return _words(pyrpo.apply_mds(_vals(a[:12])))

    def solved(target):
        """eleven words drawn, the twelfth solved for: row i mod 12 sums to `target` mod p"""
        def make(r, i):
            m, k = i % 12, r.randrange(12)
            s = _state(r)
            s[k] = 0
            s[k] = (target - _mds_sums(s)[m]) * pow(pyrpo.MDS_ROW[(k - m) % 12], -1, P) % P
            return s
        return make

    def mds_classes(o):
        o.add("each edge value", [[e] * 12 for e in E8], lambda a, i: len(set(a)) == 1 and a[0] in E8)
        o.gen("edge values crossed", nm, lambda r, i: _edge_state(r), lambda a, i: all(w in E8 for w in a))
        o.add("all p-1: the largest sum", [[P - 1] * 12], lambda a, i: all(s == 160 * (P - 1) for s in _mds_sums(a)))
        o.add("all zero", [[0] * 12], lambda a, i: not any(_mds_sums(a)))
        o.gen("sum = k p, k > 0", nm, solved(0), lambda a, i: _mds_sums(a)[i % 12] > 0 and _mds_sums(a)[i % 12] % P == 0)
        o.gen("sum = k p - 1", nm, solved(P - 1), lambda a, i: _mds_sums(a)[i % 12] % P == P - 1)
        o.gen("high word 0", nm, lambda r, i: [r.getrandbits(r.randrange(1, 57)) for _ in range(12)],
              lambda a, i: all(s >> 64 == 0 for s in _mds_sums(a)))
        o.gen("high word 159", nm, lambda r, i: [P - 1 - r.getrandbits(r.randrange(1, 57)) for _ in range(12)],
              lambda a, i: all(s >> 64 == 159 for s in _mds_sums(a)))
        o.gen("uniform", nm, lambda r, i: _state(r), lambda a, i: all(w < P for w in a))

    mds_classes(op("apply_mds", 0, 12, 12, lambda a, o, i: _eq(o[:12], mds_want(a))))
    mds_classes(op("mds_wide (sixteen lanes) + apply_mds", 100, 12, 24,
                   lambda a, o, i: _all(_tag("mds_wide", _eq(o[:12], mds_want(a))), _tag("apply_mds", _eq(o[12:24], mds_want(a))))))
    mds_classes(op("mds_wide (coin Wide)", 101, 16, 16,
                   lambda a, o, i: _all(_eq(o[:12], mds_want(a)), _tag("pos and pad", _eq(o[12:], [4, 0, 0, 0])))))

    # ---- the S-boxes on one element
    def sbox_classes(o, e):
        o.add("word edges", [[w] for w in EC], lambda a, i: a[0] < P)
        o.add("fixed points 0, 1, p-1", [[_word(x)] for x in (0, 1, P - 1)], lambda a, i, e=e: _val(a[0]) in (0, 1, P - 1) and pow(_val(a[0]), e, P) == _val(a[0]))
        o.gen("small order", n1, lambda r, i: [_word(pow(7, (P - 1) // d * r.randrange(1, d), P)) for d in [r.choice(UNITY_ORDERS)]],
              lambda a, i: _val(a[0]) != 1 and any(pow(_val(a[0]), d, P) == 1 for d in UNITY_ORDERS))
        o.gen("uniform", n1, lambda r, i: [canon(r)], lambda a, i: a[0] < P)

    sbox_classes(op("pow7", 1, 1, 1, lambda a, o, i: _eq(o[:1], [_word(pow(_val(a[0]), 7, P))])), 7)
    sbox_classes(op("pow_inv7", 2, 1, 1, lambda a, o, i: _eq(o[:1], [_word(pow(_val(a[0]), pyrpo.INV7, P))])), pyrpo.INV7)

    def inv7_all(a, o, i):
        want = [_word(pow(x, pyrpo.INV7, P)) for x in _vals(a[:12])]
        return _all(_tag("pow_inv7_all", _eq(o[:12], want)), _tag("twelve pow_inv7", _eq(o[12:24], want)))
    o = op("pow_inv7_all", 3, 12, 24, inv7_all)
    o.add("each edge value", [[e] * 12 for e in E8], lambda a, i: len(set(a)) == 1 and a[0] in E8)
    o.gen("edge values crossed", nm, lambda r, i: _edge_state(r), lambda a, i: all(w in E8 for w in a))
    o.gen("fixed points crossed", nm, lambda r, i: [_word(r.choice((0, 1, P - 1))) for _ in range(12)],
          lambda a, i: all(x in (0, 1, P - 1) for x in _vals(a)))
    o.gen("uniform", nm, lambda r, i: _state(r), lambda a, i: all(w < P for w in a))

    # ---- gl::add(s, RC) and the S-box behind it, as the rounds use them: the twelve lanes of round r
    assert all(c >= 1 << 32 for c in pyrpo.RC0_MONT + pyrpo.RC1_MONT)       # so that every class below exists for every constant
    for kind, code, rc_words, rc_vals, e in (("rc0+pow7", 4, pyrpo.RC0_MONT, pyrpo.RC0, 7), ("rc1+pow_inv7", 5, pyrpo.RC1_MONT, pyrpo.RC1, pyrpo.INV7)):
        for rnd in range(7):
            rc, rv = rc_words[12 * rnd:12 * rnd + 12], rc_vals[12 * rnd:12 * rnd + 12]
            o = op("%s[round %d]" % (kind, rnd), code, 12, 12,
                   lambda a, o, i, rv=rv, e=e: _eq(o[:12], [_word(pow((x + c) % P, e, P)) for x, c in zip(_vals(a[:12]), rv)]), aux=rnd)
            o.add("s + RC = p", [[P - c for c in rc]], lambda a, i, rc=rc: all(s + c == P for s, c in zip(a, rc)))
            o.add("s + RC = p - 1", [[P - 1 - c for c in rc]], lambda a, i, rc=rc: all(s + c == P - 1 for s, c in zip(a, rc)))
            o.gen("s + RC wraps 2^64", n, lambda r, i, rc=rc: [r.randrange((1 << 64) - c, P) for c in rc],
                  lambda a, i, rc=rc: all(s < P and s + c > M64 for s, c in zip(a, rc)))
            o.gen("p <= s + RC < 2^64", n, lambda r, i, rc=rc: [r.randrange(P - c, (1 << 64) - c) for c in rc],
                  lambda a, i, rc=rc: all(s < P and P <= s + c <= M64 for s, c in zip(a, rc)))
            o.gen("s + RC < p", n, lambda r, i, rc=rc: [r.randrange(P - c) for c in rc], lambda a, i, rc=rc: all(s + c < P for s, c in zip(a, rc)))
            o.gen("edge values crossed", n, lambda r, i: _edge_state(r), lambda a, i: all(w in E8 for w in a))

    # ---- the whole permutation in every device form (field_prims.hip, op 200), on full 12-element states
    def forms(a, o, i):
        a = a[:12]
        want = _words(pyrpo.permute(_vals(a)))
        want0 = want[4:8] if not any(a[:4]) else _words(pyrpo.permute([0] * 4 + _vals(a[4:])))[4:8]
        return _all(_tag("msrpo::permute", _eq(o[0:12], want)), _tag("coin Wide", _eq(o[12:24], want)), _tag("coin Narrow", _eq(o[24:36], want)),
                    _tag("rpo256_merge_level_wide on the rate words", _eq(o[36:40], want0)), _tag("pos after Wide, Narrow", _eq(o[40:42], [4, 4])),
                    _tag("Wide against msrpo::permute", _eq(o[12:24], o[0:12])), _tag("Narrow against msrpo::permute", _eq(o[24:36], o[0:12])),
                    _tag("sixteen lanes against msrpo::permute", _eq(o[36:40], o[4:8])) if not any(a[:4]) else None)
    o = op("permute: msrpo::permute, coin Wide, coin Narrow, sixteen lanes", 200, 12, 42, forms)
    o.add("each edge value", [[e] * 12 for e in E8], lambda a, i: len(set(a)) == 1 and a[0] in E8)
    o.add("all zero, all p-1", [[0] * 12, [P - 1] * 12])
    o.gen("edge values crossed", np_, lambda r, i: _edge_state(r), lambda a, i: all(w in E8 for w in a))
    o.gen("zero capacity, edge rate", np_, lambda r, i: [0] * 4 + _edge_state(r)[4:], lambda a, i: not any(a[:4]) and all(w in E8 for w in a))
    o.gen("zero capacity, uniform rate", np_, lambda r, i: [0] * 4 + _state(r)[4:], lambda a, i: not any(a[:4]) and all(w < P for w in a))
    o.gen("capacity 1, 0, 0, 0: a padded row", np_, lambda r, i: [_word(1), 0, 0, 0] + _state(r)[4:], lambda a, i: _vals(a[:4]) == [1, 0, 0, 0])
    o.gen("non-zero capacity, uniform", np_, lambda r, i: _state(r), lambda a, i: all(a[:4]) and all(w < P for w in a))
    return ops


_BUILDERS = {"gl": _gl, "gld": _gld, "limb": _limb, "acc": _acc, "f252": _f252, "rpo": _rpo}


def ops(family, n):
    """every op of a family, `n` inputs per drawn class (fixed classes such as crossed edges come on top)"""
    return _BUILDERS[family](n)


# ---- one build in a process of its own ---------------------------------------------------------------------------------------
def save_inputs(path, all_ops):
    arrs = {"count": np.array(len(all_ops))}
    for j, o in enumerate(all_ops):
        arrs["meta%d" % j] = np.array([FAMILIES.index(o.family), o.code, o.aux, o.os], dtype=np.int64)
        arrs["in%d" % j] = o.inputs()
        arrs["tab%d" % j] = o.tab()
    np.savez(path, **arrs)


def _main(argv):
    if len(argv) != 5 or argv[1] != "device":
        print(__doc__)
        return 2
    lib = Lib(argv[2])
    d = np.load(argv[3])
    res = {}
    for j in range(int(d["count"])):
        fam, code, aux, os_ = (int(x) for x in d["meta%d" % j])
        try:
            res["out%d" % j] = lib.run_raw(FAMILIES[fam], code, aux, d["in%d" % j], os_, d["tab%d" % j])
        except RuntimeError as e:                  # a failing entry ends the run: nothing more is launched
            print("field_prims:", e, flush=True)
            np.savez(argv[4], **res)
            return 1
    np.savez(argv[4], **res)
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv))
