"""The prover with hash="keccak256" / "sha3_256" (pipeline.prove, both fields): every root recomputed from the downloaded LDEs and
FRI layers with tests/keccak_ref.py (hashlib for SHA3-256), every opening verified against its root, the nonce from a host search and
every coin draw from a host replay of the transcript; the column-sharded LDE commitment (lde_commit_sharded) over 2 ranks against the
single-device root, and distributed.prove_sharded(hash="keccak256") over the same 2 ranks against prove_phases; the
C++ mirror's Hash::Keccak256 / Hash::Sha3_256 against the Python mirror."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref
from tests import backends, coin_ref, keccak_ref
from tests.test_blake2s import _row_bytes
from tests.test_blake2s_prover import _splitmix
from tests.test_keccak import _pow_search, _verify, hmany
from tests.test_prove_transcript import BITS, BLOWUP, FOLDING, MAXREM, NQ, SEED, setup
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3, STARK252_FP as F252, GpuVec, Matrix, MerkleTree, grind_proof_of_work, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = {FP: 1, GOLDILOCKS_FQ3: 3, F252: 4}


def _root(variant, leaves):
    level = list(leaves)
    while len(level) > 1:
        level = hmany(variant, [level[2 * i] + level[2 * i + 1] for i in range(len(level) // 2)])
    return level[0]


def _matrix_root(variant, field, cols):
    cols = [np.asarray(c) for c in cols]
    n = len(cols[0]) // WORDS[field]
    return _root(variant, hmany(variant, _row_bytes(field, cols, n)))


def _replay(out, field, variant):
    """the verifier's side of the transcript with the helper's coin -> every draw, as canonical integers"""
    rf = coin_ref.FP252 if field == F252 else coin_ref.FP
    ints = lambda words: pipeline.from_mont_words(field, words)              # noqa: E731
    mont = lambda values: pipeline.to_mont_words(field, values).ravel()      # noqa: E731
    c = keccak_ref.Coin(SEED, variant)
    got = {}
    c.reseed_digest(out["base_root"])
    got["challenges"] = ints(c.draw(rf, len(out["challenges"])))
    c.reseed_digest(out["composition_root"])
    got["z"] = ints(c.draw(rf, 1))[0]
    c.reseed_elements(rf, mont(list(out["ood"][0]) + list(out["ood"][1])))
    nexec, ncomp = len(out["ood"][0]), len(out["ood"][1])
    d = ints(c.draw(rf, nexec + ncomp + 2))
    got["deep"] = (d[:nexec], d[nexec: nexec + ncomp], (d[-2], d[-1]))
    got["fri_alphas"] = []
    for root in out["fri_roots"]:
        c.reseed_digest(root)
        got["fri_alphas"].append(ints(c.draw(rf, 1))[0])
    c.reseed_elements(rf, out["remainder_coeffs"])
    got["nonce"] = c.grind(BITS)
    c.reseed_int(out["nonce"])
    got["positions"] = c.draw_queries(NQ, len(out["remainder"]) * FOLDING ** len(out["fri_roots"]))
    return got


def _run(kind, field, log_t, variant):
    pl, trace, comp, ce, nch, hints = setup(kind, field, log_t)
    out = pipeline.prove(pl, trace, comp, nch, hints, SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash=variant, ce_blowup=ce, field=field, keep=True)
    V = WORDS[field]
    mats = lambda k: [c.to_numpy() for c in out[k].columns]                  # noqa: E731
    # roots, from the downloaded values
    assert out["base_root"] == _matrix_root(variant, field, mats("lde"))
    assert out["composition_root"] == _matrix_root(variant, field, mats("comp_lde"))
    assert len(out["fri_roots"]) == pipeline.fri_num_layers((1 << log_t) * BLOWUP, BLOWUP, FOLDING, MAXREM) >= 1
    for layer, root in zip(out["fri_layers"], out["fri_roots"]):
        rows = layer.to_numpy().reshape(-1, FOLDING, V)
        assert root == _matrix_root(variant, field, [np.ascontiguousarray(rows[:, k, :]).ravel() for k in range(FOLDING)])
    # every coin draw and the proof-of-work, from the host replay
    got = _replay(out, field, variant)
    assert out["challenges"] == got["challenges"] and out["z"] == got["z"]
    assert (out["deep"].execution_trace, out["deep"].composition_trace, out["deep"].degree) == got["deep"]
    assert out["fri_alphas"] == got["fri_alphas"]
    assert out["nonce"] == got["nonce"]
    assert out["positions"] == got["positions"] and 1 <= len(got["positions"]) <= NQ
    # openings lead to the roots
    q = out["queries"]
    assert _verify(variant, out["base_root"], q.base_trace_proof, out["positions"])
    assert _verify(variant, out["composition_root"], q.composition_trace_proof, out["positions"])
    for opening, root in zip(out["fri_openings"], out["fri_roots"]):
        assert _verify(variant, root, opening["proof"], opening["positions"])
    return out


EMU_CASES = [(FP, 7, "keccak256"), (F252, 7, "keccak256"), (F252, 7, "sha3_256")]


@pytest.mark.parametrize("field,log_t,variant", EMU_CASES, ids=["goldilocks-keccak256", "fp252-keccak256", "fp252-sha3_256"])
def test_prover_keccak_emu(field, log_t, variant):
    _run("emu", field, log_t, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("field,variant", [(FP, "keccak256"), (F252, "keccak256"), (F252, "sha3_256")],
                         ids=["goldilocks-keccak256", "fp252-keccak256", "fp252-sha3_256"])
def test_prover_keccak_hip(field, variant):
    """2^12 rows x 8 columns"""
    _run("hip", field, 12, variant)


def test_names_are_still_refused_where_they_were():
    pl, trace, comp, ce, nch, hints = setup("emu", F252, 4)
    with pytest.raises(ValueError, match="RPO-256"):
        pipeline.prove(pl, trace, comp, nch, hints, SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash="rpo256", ce_blowup=ce, field=F252)
    assert pipeline.pow_hash("keccak256") == "keccak256" and pipeline.pow_hash("sha3_256") == "sha3_256"
    assert pipeline.pow_hash("rpo256") == "sha256" and pipeline.pow_hash("blake2s") == "blake2s"


def test_sharded_keccak_commit_matches_single_device_gloo(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dist_keccak_worker import PROVE, SHAPES, prove_inputs
    world = 2
    port = str(29400 + (os.getpid() % 400))
    procs, files = [], []
    for r in range(world):
        f = str(tmp_path / f"r{r}.txt")
        files.append(f)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_keccak_worker.py"), str(r), str(world), port, f],
                                      cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=300)
        assert p.returncode == 0, out.decode()[-2000:]
    pl = backends.planner("emu")
    want = []
    for name, V, total_cols, log_n, log_b, variant in SHAPES:
        field = GOLDILOCKS_FQ3 if name == "fq3" else FP
        cols = [cref.lde(cref.random_elements((1 << log_n) * V, 3000 + c), log_n, log_b, V, 7, True) for c in range(total_cols)]
        root = MerkleTree.from_matrix(Matrix.from_numpy(pl, cols, field), variant).root()
        assert root == _matrix_root(variant, field, cols)
        want.append(root.hex())
    # prove_sharded: the base root is the helper's over the single-device LDE, the nonce a host search from the last FRI root
    log_rows, ncols, blowup, folding, max_rem, bits, _, variant = PROVE
    cols, comp, ce, draws = prove_inputs()
    one = pipeline.prove_phases(pl, Matrix.from_numpy(pl, cols, FP), comp, draws, blowup, folding, max_rem, bits, hash=variant, ce_blowup=ce, keep=True)
    assert one["base_root"] == _matrix_root(variant, FP, [c.to_numpy() for c in one["lde"].columns])
    assert one["nonce"] == _pow_search(variant, one["fri_roots"][-1], bits)
    want.append(f"prove:ok:{one['base_root'].hex()}:{one['fri_roots'][-1].hex()}")
    for f in files:
        assert open(f).read().split("\n") == want


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------------

SRC = os.path.join(ROOT, "tests", "cpp", "test_keccak_mirror.cpp")


def _binary(kind):
    if kind == "emu":
        sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
        import build_emu
        so, exe, extra = build_emu.build(), os.path.join(ROOT, "tests", "cpp", "_build", "test_keccak_mirror_emu"), []
    else:
        from ministark_amd import build
        so, exe = build.build(verbose=False), os.path.join(ROOT, "tests", "cpp", "_build", "test_keccak_mirror")
        extra = ["-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)] + extra)
    return exe


def _python_cases(pl):
    from ministark_amd.coin import PublicCoin
    out = []
    for variant in ("keccak256", "sha3_256"):
        for name, field, n, ncols, seed in (("fp_1x256", FP, 256, 1, 11), ("fp_17x256", FP, 256, 17, 21), ("fq3_6x128", GOLDILOCKS_FQ3, 128, 6, 41)):
            V = WORDS[field]
            m = Matrix.from_numpy(pl, [_splitmix(n * V, seed + c) for c in range(ncols)], field)
            out.append({"case": f"{variant}_{name}", "root": MerkleTree.from_matrix(m, variant).root().hex()})
        ev = GpuVec.from_numpy(pl, _splitmix(1 << 10, 51), FP)
        out.append({"case": f"{variant}_fri_fp_8", "root": MerkleTree.from_fri_layer(ev, 8, variant).root().hex()})
        seed = bytes((i * 13 + 1) & 0xFF for i in range(32))
        coin = PublicCoin(pl, seed, variant)
        coin.reseed_int(5)
        out.append({"case": f"{variant}_pow", "nonce": grind_proof_of_work(pl, seed, 9, hash=variant), "sha256": grind_proof_of_work(pl, seed, 9),
                    "coin_nonce": coin.grind(9), "coin_word": int(coin.draw(FP, 1).to_numpy()[0])})
    return out


@pytest.mark.parametrize("kind", [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)])
def test_cpp_mirror_matches_python(kind):
    exe = _binary(kind)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "cpp keccak mirror ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    cpp = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    py = _python_cases(backends.planner(kind))
    assert cpp == py
    fp1 = _splitmix(256, 11)
    assert cpp[0]["root"] == _matrix_root("keccak256", FP, [fp1]).hex()
    # and against the helper's coin: reseed_int(5), grind 9 bits, one Goldilocks draw
    seed = bytes((i * 13 + 1) & 0xFF for i in range(32))
    for variant in ("keccak256", "sha3_256"):
        case = [c for c in cpp if c["case"] == f"{variant}_pow"][0]
        ref = keccak_ref.Coin(seed, variant)
        assert case["nonce"] == ref.grind(9)
        ref.reseed_int(5)
        assert case["coin_nonce"] == ref.grind(9) and [case["coin_word"]] == ref.draw(coin_ref.FP, 1)
