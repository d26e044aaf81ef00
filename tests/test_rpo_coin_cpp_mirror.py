"""The C++ host mirror of the RPO-256 public coin (tests/cpp/test_rpo_coin_mirror.cpp): three FRI layers through ms::RpoCoin,
MerkleTree::root_ptr of RPO-256 trees and the device-alpha apply_drp.  The program prints its roots, alphas, remainder, state, nonce,
two Fq3 draws and positions (Montgomery words); tests/rpo_coin_ref.py replays the transcript from the roots and the remainder and must
arrive at the same alphas, state, nonce, draws and positions."""
import os
import subprocess
import sys

import pytest

from tests import rpo_coin_ref
from ministark_amd.api import GL_P, gl_from_mont

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_rpo_coin_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def _check(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "rpo coin host mirror ok" in out.stdout, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    rows = lambda tag: [[gl_from_mont(int(v)) for v in rest] for t, *rest in lines if t == tag]
    roots, alphas = rows("root"), rows("alpha")
    assert len(roots) == len(alphas) == 3 and all(len(r) == 4 for r in roots)
    c = rpo_coin_ref.Coin([5, 6, 7, GL_P - 1])
    for root, alpha in zip(roots, alphas):
        c.reseed_digest(root)
        assert c.draw(1) == alpha
    remainder = rows("remainder")[0]
    assert len(remainder) == (1 << 9) // 4 ** 3
    c.reseed_elements(remainder)
    assert c.state() == {"s": rows("state")[0], "pos": 4}
    nonce = int([rest for t, *rest in lines if t == "nonce"][0][0])
    assert nonce == c.grind(8)
    c.reseed_int(nonce)
    assert c.s[0] & 0xFF == 0
    assert c.draw(6) == rows("fq3")[0]
    assert [int(rest[0]) for t, *rest in lines if t == "position"] == c.draw_queries(8, 1 << 9)


def test_rpo_coin_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_rpo_coin_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe)


@pytest.mark.gpu
def test_rpo_coin_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_rpo_coin_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe)
