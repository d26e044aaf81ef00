"""The C++ host mirror of the extension columns (tests/cpp/test_extension_mirror.cpp): ms::build_extension_columns over Fp -> Fq3 and
Fp -> Fp, and ms::DeepPolyComposer<ms::Fp> with a non-null extension matrix, against the Python mirror on the same backend and the same
inputs (one generator, restated here), word for word."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import backends
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, ExtColumn, GpuVec, Matrix, build_extension_columns
from ministark_amd.api import GL_P, gl_from_mont
from ministark_amd.composer import DeepCompositionCoeffs, DeepPolyComposer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_extension_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
COLUMNS = [ExtColumn(1, [(+1, 0, None), (-1, 1, 0, 0), (-1, 2, 1, 1)], [], mask=("nonzero", 3)),
           ExtColumn(("challenge", 1), [(+1, 3, None)], [(+1, None, 0, 1)], inclusive=True),
           ExtColumn(0, [], [(-1, None, 2, -7), (+1, None, None)])]


class Lcg:
    def __init__(self):
        self.s = 42

    def words(self, n):
        out = []
        for _ in range(n):
            self.s = (self.s * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
            out.append((self.s >> 1) % GL_P)
        return np.array(out, dtype=np.uint64)


def _check(exe, kind):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "extension host mirror ok" in run.stdout, run.stdout + run.stderr
    got = {}
    for line in run.stdout.splitlines():
        tag, *rest = line.split()
        if tag in ("fq3", "fp", "ood_exec", "ood_comp", "deep"):
            got[(tag, int(rest[0]))] = np.array([int(v) for v in rest[1:]], dtype=np.uint64)
    pl, g, n, m = backends.planner(kind), Lcg(), 300, 256
    base = Matrix([GpuVec.from_numpy(pl, g.words(n), FP) for _ in range(4)])
    chal3, chal1 = GpuVec.from_numpy(pl, g.words(12), FQ3F), GpuVec.from_numpy(pl, g.words(4), FP)
    ext3 = build_extension_columns(pl, base, chal3, COLUMNS, FQ3F).to_numpy()
    ext1 = build_extension_columns(pl, base, chal1, COLUMNS, FP).to_numpy()
    for c in range(3):
        assert np.array_equal(got[("fq3", c)], ext3[c]) and np.array_equal(got[("fp", c)], ext1[c]), c
    # DeepPolyComposer<Fp> with an extension matrix
    bp, ep, cp = (Matrix([GpuVec.from_numpy(pl, g.words(m), FP) for _ in range(k)]) for k in (4, 2, 1))
    args = [(c, o) for c in range(6) for o in (0, 1)]
    z = int(g.words(1)[0])
    composer = DeepPolyComposer(args, m, z, bp, ep, cp)
    execution, composition = composer.get_ood_evals()
    assert [int(v) for v in got[("ood_exec", 0)]] == [int(v) for v in execution]
    assert [int(v) for v in got[("ood_comp", 0)]] == [int(v) for v in composition]
    ints = lambda k: [int(v) for v in g.words(k)]
    coeffs = DeepCompositionCoeffs(ints(len(args)), ints(1), tuple(ints(2)))
    deep = composer.into_deep_poly(coeffs).to_numpy()
    assert np.array_equal(got[("deep", 0)], deep) and len(deep) == m and any(gl_from_mont(int(v)) for v in deep)


def test_extension_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_extension_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe, "emu")


@pytest.mark.gpu
def test_extension_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_extension_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe, "hip")
