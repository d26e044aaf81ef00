"""The C++ host mirror of the range check (tests/cpp/test_range_mirror.cpp): ms::limb_decompose and ms::range_multiplicities over Fp and
Fp252 against values the loops of tests/range_ref.py give.  This driver dumps, per field, the trace (Montgomery words), the specs and sets,
and the expected columns, m column and reports into a file; the program runs the calls on them and compares."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import range_ref
from tests.test_limb_decompose import FIELDS, mask_column, values
from ministark_amd import LimbSpec, RangeSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_range_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
_KIND = {None: 0, "nonzero": 1, "zero": 2}
SHAPES = {"fp": (12, 5), "fp252": (28, 8)}                                      # limbs across word boundaries; fewer bits than either field has
TABLE_BITS, N = 10, 300


def _dump(path):
    """300 rows: a masked decomposition whose limbs straddle words and overflow, then the first two limb columns counted against a table of
    2^10 rows -- narrower than a limb, so some limbs are missing -- into an m column of 1030 elements"""
    with open(path, "w") as f:
        for fname in ("fp", "fp252"):
            pair, (bits, nlimbs) = FIELDS[fname], SHAPES[fname]
            rng = np.random.default_rng(N)
            base = [values(pair, rng, bits, nlimbs, N), mask_column(rng, N)] + [[0] * N for _ in range(nlimbs)]
            specs = [LimbSpec(0, 2, nlimbs, bits, ("nonzero", 1))]
            sets = [RangeSet(2), RangeSet(3, ("zero", 1)), RangeSet(3, ("nonzero", 1))]
            n_m = (1 << TABLE_BITS) + 6
            after, lrep = range_ref.limb_decompose(base, specs)
            m, rrep = range_ref.range_multiplicities(after, TABLE_BITS, sets, n_m)
            assert lrep["overflow"] > 0 and 0 < lrep["active"] < N and rrep["missing"] > 0 and sum(m) > 50 and max(m) > 1
            f.write(f"{N} {len(base)} {len(specs)} {TABLE_BITS} {len(sets)} {n_m}\n")
            mask = lambda mk: [_KIND[None], 0] if mk is None else [_KIND[mk[0]], mk[1]]
            for sp in specs:
                f.write(" ".join(str(v) for v in [sp.src, sp.dst0, sp.nlimbs, sp.bits] + mask(sp.mask)) + "\n")
            for st in sets:
                f.write(" ".join(str(v) for v in [st.col] + mask(st.mask)) + "\n")
            for c in base + after + [None, m]:
                if c is None:
                    f.write(" ".join(str(lrep[k]) for k in ("overflow", "first_overflow_spec", "first_overflow_row", "active")) + "\n")
                else:
                    f.write(" ".join(str(int(w)) for w in pair.base_words(c)) + "\n")
            f.write(" ".join(str(rrep[k]) for k in ("missing", "first_missing_set", "first_missing_row")) + "\n")


def _check(exe, name):
    data = os.path.join(OUT, name + ".txt")
    _dump(data)
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "range host mirror ok" in run.stdout, run.stdout + run.stderr
    assert "fp rows 300" in run.stdout and "fp252 rows 300" in run.stdout


def test_range_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_range_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe, "range_mirror_emu")


@pytest.mark.gpu
def test_range_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_range_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe, "range_mirror")
