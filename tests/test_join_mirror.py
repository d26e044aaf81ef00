"""The C++ host mirror of the row join (tests/cpp/test_join_mirror.cpp): ms::join_rows and ms::fetch_columns over Fp and Fp252 against
values the loop of tests/join_ref.py gives.  This driver dumps, per field, the inputs (Montgomery words, the keys) and the expected match
arrays, report and fetched payload column into a file; the program runs the calls on them and compares."""
import os
import subprocess
import sys

import pytest

from tests.join_ref import NONE, REPORT_FIELDS
from tests.test_join_rows import FIELDS, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_join_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
_KIND = {None: 0, "nonzero": 1, "zero": 2}
PAYLOAD = 4                                                                     # layout(): the column after the table's key and mask columns


def _dump(path):
    """duplicate-heavy, three sets, every mask kind, missing keys: 300 rows against a 120-row table over Fp, then the same over Fp252"""
    with open(path, "w") as f:
        for fname in ("fp", "fp252"):
            pair = FIELDS[fname]
            table, base, table_key, keys, match, rep = case(fname, 120, 300, 2, 3, 40, "nonzero", ("zero", None, "nonzero"))
            assert rep["missing"] > 0 and rep["duplicate_table_rows"] > 0 and 0 < rep["table_active"] < 120 and len(table) == PAYLOAD + 1
            f.write(f"{len(table[0])} {len(table)} {len(base[0])} {len(base)} {len(table_key.cols)} {len(keys)} {PAYLOAD}\n")
            for t in [table_key] + keys:
                kind, col = (None, 0) if t.mask is None else t.mask
                f.write(" ".join(str(v) for v in t.cols + [_KIND[kind], col]) + "\n")
            for c in table + base:
                f.write(" ".join(str(int(w)) for w in pair.base_words(c)) + "\n")
            for m in match:
                f.write(" ".join(str(v) for v in m) + "\n")
            f.write(" ".join(str(rep[k]) for k in ("matched", "missing", "first_missing_set", "first_missing_row", "duplicate_table_rows", "table_active")) + "\n")
            assert set(REPORT_FIELDS) == set(rep)
            f.write(" ".join(str(int(w)) for w in pair.base_words([0 if j == NONE else table[PAYLOAD][j] for j in match[0]])) + "\n")


def _check(exe, name):
    data = os.path.join(OUT, name + ".txt")
    _dump(data)
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "join host mirror ok" in run.stdout, run.stdout + run.stderr
    assert "fp rows 300 table 120" in run.stdout and "fp252 rows 300 table 120" in run.stdout


def test_join_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_join_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe, "join_mirror_emu")


@pytest.mark.gpu
def test_join_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_join_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe, "join_mirror")
