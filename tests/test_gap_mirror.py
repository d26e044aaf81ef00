"""The C++ host mirror of the padded-table layer (tests/cpp/test_gap_mirror.cpp): ms::sort_rows -> ms::gap_plan -> ms::gap_fill over Fp and
Fp252 against values the loops of tests/sort_ref.py and tests/gaps_ref.py give -- which the Python mirror is compared with in
tests/test_gap_rows.py.  This driver dumps, per field, the inputs (Montgomery words, the sort key, the spec, the column records) and the
expected start, report and filled columns into a file; the program runs the calls on them and compares."""
import os
import subprocess
import sys

import pytest

from tests import gaps_ref
from tests.sort_ref import reference
from tests.test_gap_rows import FIELDS, MEMORY, REPORT
from ministark_amd import GapSpec, SortKey
from ministark_amd.extension import _GAP_KIND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_gap_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
N_OUT = 2048


def _dump(path):
    """a memory table over Fp, then over Fp252: 300 processor rows of `pipeline.memory_processor_rows`, the rows whose instr is not 0 sorted
    by (mp, cycle), gaps filled, padded to 2048"""
    from ministark_amd import pipeline
    with open(path, "w") as f:
        for fname in ("fp", "fp252"):
            pair = FIELDS[fname]
            base = pipeline.memory_processor_rows(299, 5)
            key, spec = SortKey([1, 0], mask=("nonzero", 3)), GapSpec(group=[1], counter=0, mask=("nonzero", 3))
            perm, _ = reference(base, key, 8 * pair.bf.nlimbs)
            start, rep = gaps_ref.plan(base, spec, perm)
            assert rep["gaps"] > 2 and rep["unordered"] == 0 and 300 < rep["rows_out"] < N_OUT
            want = gaps_ref.fill(base, start, MEMORY, N_OUT, pair.bf.p, perm)
            f.write(f"{len(base[0])} {len(base)} {len(MEMORY)} {N_OUT}\n")
            for c in base:
                f.write(" ".join(str(int(w)) for w in pair.base_words(c)) + "\n")
            f.write(" ".join(str(v) for v in start) + "\n")
            f.write(" ".join(str(rep[k]) for k in REPORT) + " 0\n")          # and pad0
            f.write(" ".join(f"{_GAP_KIND[k]} {0 if s is None else s}" for k, s in MEMORY) + "\n")
            for c in want:
                f.write(" ".join(str(int(w)) for w in pair.base_words(c)) + "\n")


def _check(exe, name):
    data = os.path.join(OUT, name + ".txt")
    _dump(data)
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "gap host mirror ok" in run.stdout, run.stdout + run.stderr
    assert "fp rows 300" in run.stdout and "fp252 rows 300" in run.stdout


def test_gap_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_gap_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe, "gap_mirror_emu")


@pytest.mark.gpu
def test_gap_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_gap_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe, "gap_mirror")
