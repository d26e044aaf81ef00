"""The C++ host mirror of the row sort (tests/cpp/test_sort_mirror.cpp): ms::sort_rows and ms::permute_columns over Fp and Fp252 against
values the loop of tests/sort_ref.py gives -- which the Python mirror is compared with in tests/test_sort_rows.py.  This driver dumps, per
field, the inputs (Montgomery words, the key) and the expected permutation and report into a file; the program runs the calls on them and
compares."""
import os
import subprocess
import sys

import pytest

from tests.sort_ref import reference
from tests.test_sort_rows import FIELDS, masked_key, random_base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_sort_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
_KIND = {None: 0, "nonzero": 1, "zero": 2}


def _dump(path):
    """ties on the leading components, a mask: 300 rows over Fp, then 300 over Fp252"""
    with open(path, "w") as f:
        for fname in ("fp", "fp252"):
            pair = FIELDS[fname]
            base, key = random_base(fname, 300, 3, True), masked_key(3, "nonzero")
            perm, rep = reference(base, key, 8 * pair.bf.nlimbs)
            assert 0 < rep["active"] < 300 and rep["varying_bytes"] > 2
            f.write(f"{len(base[0])} {len(base)} {len(key.cols)}\n")
            f.write(" ".join(str(v) for v in key.cols + [_KIND[key.mask[0]], key.mask[1]]) + "\n")
            for c in base:
                f.write(" ".join(str(int(w)) for w in pair.base_words(c)) + "\n")
            f.write(" ".join(str(i) for i in perm) + "\n")
            f.write(f"{rep['active']} {rep['varying_bytes']}\n")


def _check(exe, name):
    data = os.path.join(OUT, name + ".txt")
    _dump(data)
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "sort host mirror ok" in run.stdout, run.stdout + run.stderr
    assert "fp rows 300" in run.stdout and "fp252 rows 300" in run.stdout


def test_sort_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_sort_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe, "sort_mirror_emu")


@pytest.mark.gpu
def test_sort_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_sort_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe, "sort_mirror")
