"""The prover with hash="blake2s": prove_phases against itself with "sha256" (same Draws: every output that is not a digest is the
same), every BLAKE2s root recomputed with hashlib from the downloaded LDEs and FRI layers, the nonce from a hashlib search; the
row-sharded commitment over 2 ranks against the single-device root; the C++ mirror's Hash::Blake2s against the Python mirror."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref
from tests import backends
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3, Matrix, MerkleTree, grind_proof_of_work

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cref.GL_P
M32 = np.uint64(0xFFFFFFFF)


def _from_mont(x):
    """Goldilocks Montgomery words -> canonical, vectorised (x * 2^-64 mod p, the reduction of a 128-bit value with a zero high
    half); checked against oracle.cref.from_mont on every call's first words"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        a = x + (x << np.uint64(32))
        e = (a < x).astype(np.uint64)
        b = a - (a >> np.uint64(32)) - e
        r = np.uint64(0) - b
        c = (b > 0).astype(np.uint64)
        r = r - ((np.uint64(0) - c) & M32)
    k = min(len(x), 64)
    assert np.array_equal(r[:k], cref.from_mont(x[:k]))
    return r


def _leaves(cols):
    """hashlib BLAKE2s leaves of the rows of column-major Fp columns (Montgomery words)"""
    rows = np.ascontiguousarray(np.stack([_from_mont(c) for c in cols], axis=1).astype("<u8"))
    raw = rows.view(np.uint8).reshape(len(rows), -1)
    return [hashlib.blake2s(r.tobytes()).digest() for r in raw]


def _root(leaves):
    level = leaves
    while len(level) > 1:
        level = [hashlib.blake2s(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
    return level[0]


def _lz(d):
    z = 0
    for b in d:
        if b:
            return z + 8 - b.bit_length()
        z += 8
    return z


def _run(kind, log_t, seed=4242):
    from ministark_amd import pipeline
    pl = backends.planner(kind)
    blowup, folding, ncols, bits = 4, 8, 8, 8
    n_t = 1 << log_t
    cols = [cref.random_elements(n_t, seed + c) for c in range(ncols)]
    comp, ce, nch = pipeline.fib_constraints(n_t, ncols)
    nlayers = pipeline.fri_num_layers(n_t * blowup, blowup, folding, 64)
    draws = pipeline.Draws(seed, ncols, nch, ce, 32, n_t * blowup, nlayers)
    out = {}
    for h in ("sha256", "blake2s"):
        out[h] = pipeline.prove_phases(pl, Matrix.from_numpy(pl, cols, FP), comp, draws, blowup, folding, 64, bits, hash=h, keep=True,
                                       ce_blowup=ce)
    s, b = out["sha256"], out["blake2s"]
    # every output that is not a digest is the same
    mats = lambda o, k: [c.to_numpy() for c in o[k].columns]                      # noqa: E731
    for k in ("base_polys", "lde", "comp_polys", "comp_lde", "deep_lde"):
        assert all(np.array_equal(x, y) for x, y in zip(mats(s, k), mats(b, k))), k
    assert np.array_equal(s["comp_evals"].to_numpy(), b["comp_evals"].to_numpy())
    assert all(np.array_equal(x.to_numpy(), y.to_numpy()) for x, y in zip(s["fri_layers"], b["fri_layers"]))
    assert np.array_equal(s["remainder"].to_numpy(), b["remainder"].to_numpy())
    assert np.array_equal(s["remainder_coeffs"], b["remainder_coeffs"])
    assert ([int(v) for v in s["ood"][0]], [int(v) for v in s["ood"][1]]) == ([int(v) for v in b["ood"][0]], [int(v) for v in b["ood"][1]])
    for k in ("base_trace_values", "composition_trace_values"):
        assert np.array_equal(getattr(s["queries"], k), getattr(b["queries"], k)), k
    assert [o["positions"] for o in s["fri_openings"]] == [o["positions"] for o in b["fri_openings"]]
    assert all(np.array_equal(x["rows"], y["rows"]) for x, y in zip(s["fri_openings"], b["fri_openings"]))
    # the digests differ, and each BLAKE2s root is hashlib's over the downloaded values
    assert s["base_root"] != b["base_root"]
    assert b["base_root"] == _root(_leaves(mats(b, "lde")))
    assert b["composition_root"] == _root(_leaves(mats(b, "comp_lde")))
    assert len(b["fri_roots"]) == nlayers
    for layer, root in zip(b["fri_layers"], b["fri_roots"]):
        rows = layer.to_numpy().reshape(-1, folding)
        assert root == _root(_leaves([rows[:, k] for k in range(folding)]))
    # the nonce: a hashlib search from the last FRI root; the SHA-256 prover still grinds with SHA-256
    seed_b = b["fri_roots"][-1]
    n = 1
    while _lz(hashlib.blake2s(seed_b + n.to_bytes(8, "big")).digest()) < bits:
        n += 1
    assert b["nonce"] == n
    seed_s = s["fri_roots"][-1]
    n = 1
    while _lz(hashlib.sha256(seed_s + n.to_bytes(8, "big")).digest()) < bits:
        n += 1
    assert s["nonce"] == n
    # the openings of the BLAKE2s trees are views of those trees
    pos = sorted(set(draws.positions))
    assert b["queries"].base_trace_proof == MerkleTree.from_matrix(b["lde"], "blake2s").prove(pos)


def test_prover_blake2s_emu():
    _run("emu", 7)


@pytest.mark.gpu
def test_prover_blake2s_at_size_hip():
    """configs[4]'s shape: 2^22 rows x 8 columns, blow-up 4"""
    _run("hip", 22)


def test_sharded_blake2s_commit_matches_single_device_gloo(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dist_blake2s_worker import SHAPES
    world = 2
    port = str(29000 + (os.getpid() % 400))
    procs, files = [], []
    for r in range(world):
        f = str(tmp_path / f"r{r}.txt")
        files.append(f)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_blake2s_worker.py"), str(r), str(world), port, f],
                                      cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=300)
        assert p.returncode == 0, out.decode()[-2000:]
    pl = backends.planner("emu")
    want = []
    for name, V, total_cols, log_n, log_b in SHAPES:
        field = GOLDILOCKS_FQ3 if name == "fq3" else FP
        cols = [cref.lde(cref.random_elements((1 << log_n) * V, 3000 + c), log_n, log_b, V, 7, True) for c in range(total_cols)]
        root = MerkleTree.from_matrix(Matrix.from_numpy(pl, cols, field), "blake2s").root()
        if V == 1:
            assert root == _root(_leaves(cols))
        want.append(root.hex())
    for f in files:
        assert open(f).read().split("\n") == want


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------------

SRC = os.path.join(ROOT, "tests", "cpp", "test_blake2s_mirror.cpp")


def _binary(kind):
    if kind == "emu":
        sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
        import build_emu
        so, exe, extra = build_emu.build(), os.path.join(ROOT, "tests", "cpp", "_build", "test_blake2s_mirror_emu"), []
    else:
        from ministark_amd import build
        so, exe = build.build(verbose=False), os.path.join(ROOT, "tests", "cpp", "_build", "test_blake2s_mirror")
        extra = ["-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)] + extra)
    return exe


def _splitmix(n, seed):
    """the C++ test's inputs: splitmix64 words reduced below p"""
    out, s, m = [], seed, (1 << 64) - 1
    for _ in range(n):
        s = (s + 0x9E3779B97F4A7C15) & m
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        out.append((z ^ (z >> 31)) % P)
    return np.array(out, dtype=np.uint64)


def _python_cases(pl):
    from ministark_amd import GpuVec
    out = []
    for name, field, n, ncols, seed in (("fp_1x1024", FP, 1024, 1, 11), ("fp_8x1024", FP, 1024, 8, 21), ("fp_9x512", FP, 512, 9, 31),
                                        ("fq3_3x512", GOLDILOCKS_FQ3, 512, 3, 41)):
        V = 3 if field == GOLDILOCKS_FQ3 else 1
        m = Matrix.from_numpy(pl, [_splitmix(n * V, seed + c) for c in range(ncols)], field)
        out.append({"case": name, "root": MerkleTree.from_matrix(m, "blake2s").root().hex()})
    for name, field, n, ff, seed in (("fri_fp_8", FP, 1 << 11, 8, 51), ("fri_fq3_4", GOLDILOCKS_FQ3, 1 << 10, 4, 61)):
        V = 3 if field == GOLDILOCKS_FQ3 else 1
        ev = GpuVec.from_numpy(pl, _splitmix(n * V, seed), field)
        out.append({"case": name, "root": MerkleTree.from_fri_layer(ev, ff, "blake2s").root().hex()})
    for k in range(3):
        seed = bytes((i * 13 + 5 * k + 1) & 0xFF for i in range(32))
        out.append({"case": f"pow_{k}", "blake2s": grind_proof_of_work(pl, seed, 10, hash="blake2s"), "sha256": grind_proof_of_work(pl, seed, 10)})
    return out


@pytest.mark.parametrize("kind", [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)])
def test_cpp_mirror_matches_python(kind):
    exe = _binary(kind)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "cpp blake2s mirror ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    cpp = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    py = _python_cases(backends.planner(kind))
    assert cpp == py
    fp1 = _splitmix(1024, 11)
    assert cpp[0]["root"] == _root(_leaves([fp1])).hex()
