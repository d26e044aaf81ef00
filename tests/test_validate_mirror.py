"""The C++ mirror of validate_constraints (ministark_amd/csrc/host/expr.hpp; tests/cpp/test_validate_mirror.cpp) gives the same report and
the same message as the Python mirror (ministark_amd/debug.py) on cases 1, 2 and 4 of tests/test_validate_constraints.py, under the
simulator and on the GPU."""
import json
import os
import subprocess
import sys

import pytest

from tests import backends
from tests.test_validate_constraints import _corruptions, _ext_air, fib_cols, fq_matrix, gl_matrix
from oracle.pyref.fields import FQ3, GL
from ministark_amd import pipeline
from ministark_amd.debug import ConstraintViolation, validate_constraints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_validate_mirror.cpp")


def _binary(kind):
    if kind == "emu":
        sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
        import build_emu
        so, exe, extra = build_emu.build(), os.path.join(ROOT, "tests", "cpp", "_build", "test_validate_mirror_emu"), []
    else:
        from ministark_amd import build
        so, exe = build.build(verbose=False), os.path.join(ROOT, "tests", "cpp", "_build", "test_validate_mirror")
        extra = ["-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)] + extra)
    return exe


def _py(name, cons, ch, hints, base, ext=None):
    r = validate_constraints(cons, ch, hints, base, ext, raise_on_failure=False)
    try:
        validate_constraints(cons, ch, hints, base, ext)
        thrown = ""
    except ConstraintViolation as e:
        thrown = str(e)
    return {"case": name, "failures": [list(f) for f in r.failures], "unused_columns": r.unused_columns, "unused_challenges": r.unused_challenges,
            "unused_hints": r.unused_hints, "message": r.message or "", "thrown": thrown}


def _python_cases(pl):
    out = []
    n = 1 << 10
    cols = fib_cols(n)
    out.append(_py("fib_valid", pipeline.fib_air_constraints(n), [99], [cols[7][n - 1], 12345], gl_matrix(pl, cols)))
    n = 1 << 8
    for col, row in _corruptions(n):
        cols = fib_cols(n)
        claimed = cols[7][n - 1]
        cols[col][row] = (cols[col][row] + 1) % GL.p
        out.append(_py(f"fib_corrupt_{col}_{row}", pipeline.fib_air_constraints(n), [], [claimed], gl_matrix(pl, cols)))
    g = [(11, 22, 33), (44, 55, 66)]
    b = [(r * 2654435761 + 12345) % (1 << 62) for r in range(n)]
    e = [(1, 0, 0)]
    for r in range(n - 1):
        e.append(FQ3.mul(e[-1], FQ3.sub(g[0], FQ3.mul_base(g[1], b[r]))))
    for row in (-1, 0, 77, n - 1):
        em = list(e)
        if row >= 0:
            em[row] = (em[row][0], (em[row][1] + 1) % GL.p, em[row][2])
        out.append(_py("ext_valid" if row < 0 else f"ext_corrupt_{row}", _ext_air(n), g, [], gl_matrix(pl, [b]), fq_matrix(pl, [em])))
    return out


@pytest.mark.parametrize("kind", [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)])
def test_cpp_mirror_matches_python(kind):
    exe = _binary(kind)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "cpp validate mirror ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    cpp = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    py = _python_cases(backends.planner(kind))
    assert [c["case"] for c in cpp] == [c["case"] for c in py]
    for c, p in zip(cpp, py):
        assert c == p, c["case"]
    assert any(c["failures"] for c in cpp) and any(not c["failures"] for c in cpp)
    assert all(c["thrown"] == c["message"] for c in cpp)
