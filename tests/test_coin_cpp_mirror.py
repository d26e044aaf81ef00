"""The C++ host mirror of the public coin (tests/cpp/test_coin_mirror.cpp): three FRI layers through ms::PublicCoin, MerkleTree::root_ptr
and the device-alpha apply_drp.  The program prints its roots, alphas, remainder, nonce and positions; tests/coin_ref.py replays the
transcript from the roots and the remainder and must arrive at the same alphas, seed, nonce and positions."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import coin_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_coin_mirror.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
HASHES = ["sha256", "blake2s"]


def _check(exe, hash):
    out = subprocess.run([exe, hash], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "coin host mirror ok" in out.stdout, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    get = lambda tag: [v for t, *rest in lines if t == tag for v in rest]
    roots, alphas = [bytes.fromhex(r) for r in get("root")], [int(a) for a in get("alpha")]
    assert len(roots) == len(alphas) == 3
    c = coin_ref.Coin(bytes(3 * i + 1 for i in range(32)), hash)
    for root, alpha in zip(roots, alphas):
        c.reseed_digest(root)
        assert c.draw(coin_ref.FP, 1) == [alpha]
    c.reseed_elements(coin_ref.FP, np.frombuffer(bytes.fromhex(get("remainder")[0]), dtype=np.uint64))
    assert c.seed.hex() == get("seed")[0]
    nonce = int(get("nonce")[0])
    assert nonce == c.grind(8)
    c.reseed_int(nonce)
    assert [int(p) for p in get("position")] == c.draw_queries(8, 1 << 9)


@pytest.mark.parametrize("hash", HASHES)
def test_coin_mirror_under_the_simulator(hash):
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    so = build_emu.build()
    exe = os.path.join(OUT, "test_coin_mirror_emu")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    _check(exe, hash)


@pytest.mark.gpu
@pytest.mark.parametrize("hash", HASHES)
def test_coin_mirror_on_gpu(hash):
    from ministark_amd import build
    so = build.build(verbose=False)
    exe = os.path.join(OUT, "test_coin_mirror")
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    _check(exe, hash)
