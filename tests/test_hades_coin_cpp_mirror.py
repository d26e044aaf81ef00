"""The C++ host mirror of the Poseidon public coin of the 252-bit field (tests/cpp/test_hades_coin_mirror.cpp): three FRI layers through
ms::PoseidonCoin, MerkleTree::root_ptr of Poseidon trees and the device-alpha apply_drp.  The program prints its roots, alphas,
remainder, state, nonce, three draws and positions (Montgomery words); tests/hades_coin_ref.py replays the transcript from the roots
and the remainder and must arrive at the same alphas, state, nonce, draws and positions."""
import os
import subprocess
import sys

import pytest

from tests import hades_coin_ref
from ministark_amd.api import f252_from_mont_limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hades_coin_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def _check(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "hades coin host mirror ok" in out.stdout, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]

    def rows(tag):
        return [[f252_from_mont_limbs([int(v) for v in rest[i:i + 4]]) for i in range(0, len(rest), 4)] for t, *rest in lines if t == tag]
    roots, alphas = rows("root"), rows("alpha")
    assert len(roots) == len(alphas) == 3 and all(len(r) == 1 for r in roots)
    c = hades_coin_ref.Coin(5 + (6 << 64) + (7 << 128) + (8 << 192))
    for root, alpha in zip(roots, alphas):
        c.reseed_digest(root[0])
        assert c.draw(1) == alpha
    remainder = rows("remainder")[0]
    assert len(remainder) == (1 << 8) // 4 ** 3
    c.reseed_elements(remainder)
    assert c.state() == {"digest": rows("state")[0][0], "n_draws": 0}
    nonce = int([rest for t, *rest in lines if t == "nonce"][0][0])
    assert nonce == c.grind(8)
    c.reseed_int(nonce)
    assert c.draw(3) == rows("draws")[0]
    assert [int(rest[0]) for t, *rest in lines if t == "position"] == c.draw_queries(8, 1 << 8)


def test_hades_coin_mirror_under_the_simulator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_hades_coin_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe)


@pytest.mark.gpu
def test_hades_coin_mirror_on_gpu():
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_hades_coin_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe)
