"""The C++ mirror of the canonical-form scan and of checked mode (ministark_amd/csrc/host/ministark.hpp: Matrix<F>::check_canonical,
Planner::set_checked; tests/cpp/test_canonical_mirror.cpp) reports what the planted positions say it must, and surfaces a checked-mode
refusal as its exception with the inputs untouched -- under the simulator and on the GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_canonical_mirror.cpp")


def _binary(kind):
    if kind == "emu":
        sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
        import build_emu
        so, exe, extra = build_emu.build(), os.path.join(ROOT, "tests", "cpp", "_build", "test_canonical_mirror_emu"), []
    else:
        from ministark_amd import build
        so, exe = build.build(verbose=False), os.path.join(ROOT, "tests", "cpp", "_build", "test_canonical_mirror")
        extra = ["-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)] + extra)
    return exe


# what the plants of the C++ file amount to: (count, first_col, first_row, first_word)
WANT = {"fp_clean": (0, 0, 0, 0), "fp_planted": (3, 1, 400, 0), "fq3_clean": (0, 0, 0, 0), "fq3_planted": (2, 1, 7, 0),
        "f252_clean": (0, 0, 0, 0), "f252_planted": (2, 0, 511, 0)}


@pytest.mark.parametrize("kind", [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)])
def test_cpp_mirror(kind):
    env = {k: v for k, v in os.environ.items() if k != "MS_CHECK_CANONICAL"}
    out = subprocess.run([_binary(kind)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "cpp canonical mirror ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    cases = {c["case"]: c for c in (json.loads(line) for line in out.stdout.splitlines() if line.startswith("{"))}
    assert cases["default"]["checked"] is False and cases["switched_on"]["checked"] is True
    for name, want in WANT.items():
        c = cases[name]
        assert (c["count"], c["first_col"], c["first_row"], c["first_word"]) == want, c
    r = cases["fp_into_polynomials"]
    assert r["inputs_unchanged"] and "error -1" in r["thrown"] and "canonical" in r["thrown"] and "d_columns" in r["thrown"] and "column 1, row 400" in r["thrown"], r
    r = cases["fp_sum_columns"]
    assert r["inputs_unchanged"] and "canonical" in r["thrown"] and "ms_sum_columns" in r["thrown"] and "d_cols" in r["thrown"] and "column 1, row 400" in r["thrown"], r
    assert cases["fp_clean_sum_columns"] == {"case": "fp_clean_sum_columns", "thrown": "", "inputs_unchanged": True}
    assert cases["fp_unchecked_sum_columns"]["thrown"] == ""
