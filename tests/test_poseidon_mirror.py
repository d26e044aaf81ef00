"""The C++ host mirror of the Poseidon commitments (tests/cpp/test_poseidon_mirror.cpp): ms::MerkleTree::from_matrix(m, Hash::Poseidon252),
from_fri_layer and ms::poseidon252_permute against values tests/poseidon_ref.py gives.  This driver dumps the inputs (Montgomery words)
and the expected leaves, nodes and permuted states into a file; the program runs the calls on them and compares."""
import os
import random
import subprocess
import sys

import pytest

from tests import poseidon_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_poseidon_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
P = ref.P
NROWS, NCOLS, NLAYER, FF, NSTATES = 64, 3, 256, 4, 65


def _line(values):
    return " ".join(str(w) for v in values for w in ref.to_words(v)) + "\n"


def _dump(path):
    rnd = random.Random(77)
    elem = lambda: rnd.choice([0, 1, P - 1]) if rnd.random() < 0.1 else rnd.randrange(P)      # noqa: E731
    with open(path, "w") as f:
        cols = [[elem() for _ in range(NROWS)] for _ in range(NCOLS)]
        leaves = [ref.hash_many([c[r] for c in cols]) for r in range(NROWS)]
        f.write(f"{NROWS} {NCOLS}\n" + "".join(_line(c) for c in cols) + _line(leaves) + _line(ref.merkle_nodes(leaves)))
        layer = [elem() for _ in range(NLAYER)]
        leaves = [ref.hash_many(layer[i: i + FF]) for i in range(0, NLAYER, FF)]
        f.write(f"{NLAYER} {FF}\n" + _line(layer) + _line(leaves) + _line(ref.merkle_nodes(leaves)))
        states = [elem() for _ in range(3 * NSTATES)]
        want = [x for i in range(NSTATES) for x in ref.permute(*states[3 * i: 3 * i + 3])]
        f.write(f"{NSTATES}\n" + _line(states) + _line(want))


def _check(exe, name):
    data = os.path.join(OUT, name + ".txt")
    _dump(data)
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "poseidon host mirror ok" in run.stdout, run.stdout + run.stderr
    assert f"matrix rows {NROWS} cols {NCOLS}" in run.stdout and f"layer {NLAYER} folding {FF}" in run.stdout and f"states {NSTATES}" in run.stdout


def test_poseidon_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_poseidon_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe, "poseidon_mirror_emu")


@pytest.mark.gpu
def test_poseidon_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_poseidon_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe, "poseidon_mirror")
