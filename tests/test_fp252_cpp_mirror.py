"""The C++ host mirror over the 252-bit field (tests/cpp/test_fp252_mirror.cpp): DeepPolyComposer<Fp252>'s rows form against its
coefficient form, apply_drp_rows<Fp252> against apply_drp, and an Fq = Fp composer with a non-null extension matrix against Horner
sums computed in the program -- under the simulator, and on the device."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_fp252_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fp252 host mirror ok" in out.stdout, out.stdout + out.stderr


def test_fp252_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_fp252_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _run(exe)


@pytest.mark.gpu
def test_fp252_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_fp252_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _run(exe)
