"""The C++ host mirror of the bitwise-operation columns (tests/cpp/test_bitwise_mirror.cpp): ms::bitwise_columns, ms::bitwise_table and
ms::bitwise_multiplicities over Fp and Fp252 against values the loops of tests/bitwise_ref.py give.  This driver dumps, per field, the trace
(Montgomery words), the specs, ops and sets, and the expected columns, table, m column and reports into a file; the program runs the calls
on them and compares."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bitwise_ref
from tests.test_bitwise_columns import FIELDS, mask_column, operands
from ministark_amd import BitwiseSet, BitwiseSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_bitwise_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
_KIND = {None: 0, "nonzero": 1, "zero": 2}
SHAPES = {"fp": (5, 4), "fp252": (5, 14)}                                        # (bits, nlimbs): over Fp252 limb 12 straddles bit 64
OPS, N = (bitwise_ref.XOR, bitwise_ref.AND), 300


def _dump(path):
    """300 rows: c_xor and c_and written under a mask from operands some of which do not fit, then both counted against the table of two
    ops over pairs of 5-bit limbs -- the masked-out and the overflowing rows are missing -- into an m column of 2054 elements"""
    with open(path, "w") as f:
        for fname in ("fp", "fp252"):
            pair, (bits, nlimbs) = FIELDS[fname], SHAPES[fname]
            rng = np.random.default_rng(N)
            width = bits * nlimbs
            base = [operands(pair, rng, width, N, 3), operands(pair, rng, width, N, 5), mask_column(rng, N), [7] * N, [7] * N]
            specs = [BitwiseSpec(OPS[0], 0, 1, 3, width, ("nonzero", 2)), BitwiseSpec(OPS[1], 1, 0, 4, width)]
            sets = [BitwiseSet(OPS[0], 0, 1, 3, nlimbs), BitwiseSet(OPS[1], 0, 1, 4, nlimbs, ("zero", 2)), BitwiseSet(OPS[1], 1, 1, None, nlimbs)]
            n_m = (len(OPS) << (2 * bits)) + 6
            after, crep = bitwise_ref.bitwise_columns(base, specs)
            table = bitwise_ref.bitwise_table(bits, OPS, n_m)
            m, mrep = bitwise_ref.bitwise_multiplicities(after, bits, OPS, sets, n_m)
            assert crep["overflow"] > 0 and N < crep["active"] < 2 * N and mrep["missing"] > 50 and sum(m) > 50 * nlimbs and max(m) > 1
            f.write(f"{N} {len(base)} {len(specs)} {bits} {len(OPS)} {len(sets)} {n_m}\n")
            mask = lambda mk: [_KIND[None], 0] if mk is None else [_KIND[mk[0]], mk[1]]
            for sp in specs:
                f.write(" ".join(str(v) for v in [sp.op, sp.a, sp.b, sp.dst, sp.width] + mask(sp.mask)) + "\n")
            f.write(" ".join(str(op) for op in OPS) + "\n")
            for st in sets:
                f.write(" ".join(str(v) for v in [st.op, st.a, st.b, -1 if st.c is None else st.c, st.nlimbs] + mask(st.mask)) + "\n")
            for c in base + after + [None] + table + [m]:
                if c is None:
                    f.write(" ".join(str(crep[k]) for k in ("overflow", "first_overflow_spec", "first_overflow_row", "active")) + "\n")
                else:
                    f.write(" ".join(str(int(w)) for w in pair.base_words(c)) + "\n")
            f.write(" ".join(str(mrep[k]) for k in ("missing", "first_missing_set", "first_missing_row")) + "\n")


def _check(exe, name):
    data = os.path.join(OUT, name + ".txt")
    _dump(data)
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "bitwise host mirror ok" in run.stdout, run.stdout + run.stderr
    assert "fp rows 300" in run.stdout and "fp252 rows 300" in run.stdout


def test_bitwise_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_bitwise_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe, "bitwise_mirror_emu")


@pytest.mark.gpu
def test_bitwise_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_bitwise_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe, "bitwise_mirror")
