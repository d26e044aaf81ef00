"""The C++ host mirror of the LogUp lookup columns (tests/cpp/test_logup_mirror.cpp): ms::build_logup_columns over Fp -> Fq3 and Fp -> Fp
against the Python mirror on the same backend and the same inputs (one generator, restated here), word for word -- and the Python mirror
against the sequential loop of tests/logup_ref.py, so the three agree."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import backends
from tests.logup_ref import PAIRS, reference
from tests.test_extension_mirror import Lcg
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, GpuVec, LogUpColumn, Matrix, build_logup_columns
from ministark_amd.api import gl_from_mont

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_logup_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
DEN = lambda c0, c1: [(+1, 0, None), (-1, None, c0), (-1, 1, c1)]
COLUMNS = [LogUpColumn(0, [([(+1, None, 4)], DEN(2, 3)), ([(-1, None, None)], DEN(0, 1))]),
           LogUpColumn(("challenge", 2), [([], [(+1, None, 4, 1)])], mask=("nonzero", 4), inclusive=True),
           LogUpColumn(1, [])]


def _check(exe, kind):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "logup host mirror ok" in run.stdout, run.stdout + run.stderr
    got = {}
    for line in run.stdout.splitlines():
        tag, *rest = line.split()
        if tag in ("fq3", "fp"):
            got[(tag, int(rest[0]))] = np.array([int(v) for v in rest[1:]], dtype=np.uint64)
    pl, g, n = backends.planner(kind), Lcg(), 300
    base_w = [g.words(n) for _ in range(5)]
    base_w[4][::3] = 0
    base = Matrix([GpuVec.from_numpy(pl, w, FP) for w in base_w])
    w3, w1 = g.words(12), g.words(4)
    ext3 = build_logup_columns(pl, base, GpuVec.from_numpy(pl, w3, FQ3F), COLUMNS, FQ3F).to_numpy()
    ext1 = build_logup_columns(pl, base, GpuVec.from_numpy(pl, w1, FP), COLUMNS, FP).to_numpy()
    for c in range(3):
        assert np.array_equal(got[("fq3", c)], ext3[c]) and np.array_equal(got[("fp", c)], ext1[c]), c
    # and both are the sequential loop (the generator's words are Montgomery forms)
    canon = [[gl_from_mont(int(v)) for v in w] for w in base_w]
    chal3 = [tuple(gl_from_mont(int(v)) for v in w3[3 * k: 3 * k + 3]) for k in range(4)]
    for c, want in enumerate(reference(PAIRS["fp_fq3"], canon, chal3, COLUMNS)):
        assert np.array_equal(ext3[c], PAIRS["fp_fq3"].ext_words(want)), c
    for c, want in enumerate(reference(PAIRS["fp_fp"], canon, [gl_from_mont(int(v)) for v in w1], COLUMNS)):
        assert np.array_equal(ext1[c], PAIRS["fp_fp"].ext_words(want)), c


def test_logup_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_logup_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe, "emu")


@pytest.mark.gpu
def test_logup_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_logup_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe, "hip")
