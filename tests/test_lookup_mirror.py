"""The C++ host mirror of the lookup multiplicities (tests/cpp/test_lookup_mirror.cpp): ms::lookup_multiplicities over Fp and Fp252 against
values the loop of tests/lookup_ref.py gives.  This driver dumps, per field, the inputs (Montgomery words, the tuples) and the expected m
column and report into a file; the program runs the call on them -- m in place -- and compares."""
import os
import subprocess
import sys

import pytest

from tests.test_lookup_multiplicities import FIELDS, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_lookup_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
_KIND = {None: 0, "nonzero": 1, "zero": 2}


def _dump(path):
    """duplicate-heavy, three sets, every mask kind, missing tuples: 300 rows over Fp, then 300 over Fp252"""
    with open(path, "w") as f:
        for fname in ("fp", "fp252"):
            pair = FIELDS[fname]
            base, table, lookups, out, cnt, rep = case(fname, 300, 2, 3, 40, "nonzero", ("zero", None, "nonzero"))
            assert out == len(base) - 1 and rep["missing"] > 0 and rep["duplicate_table_rows"] > 0
            f.write(f"{len(base[0])} {len(base)} {len(table.cols)} {len(lookups)}\n")
            for t in [table] + lookups:
                kind, col = (None, 0) if t.mask is None else t.mask
                f.write(" ".join(str(v) for v in t.cols + [_KIND[kind], col]) + "\n")
            for c in base:
                f.write(" ".join(str(int(w)) for w in pair.base_words(c)) + "\n")
            f.write(" ".join(str(int(w)) for w in pair.base_words(cnt)) + "\n")
            f.write(f"{rep['missing']} {rep['first_missing_set']} {rep['first_missing_row']} {rep['duplicate_table_rows']}\n")


def _check(exe, name):
    data = os.path.join(OUT, name + ".txt")
    _dump(data)
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "lookup host mirror ok" in run.stdout, run.stdout + run.stderr
    assert "fp rows 300" in run.stdout and "fp252 rows 300" in run.stdout


def test_lookup_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_lookup_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe, "lookup_mirror_emu")


@pytest.mark.gpu
def test_lookup_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_lookup_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe, "lookup_mirror")
