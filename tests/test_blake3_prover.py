"""The prover with hash="blake3_256" on the fib AIR at 2^10 rows, over Goldilocks and the 252-bit field:
  pipeline.prove         every root recomputed from the downloaded LDEs and FRI layers with tests/blake3_ref.py, every opening verified
                         against its root, the nonce from a host search and every coin draw from a host replay of the transcript;
  pipeline.prove_phases  against itself with "sha256" under the same Draws: every trace, DEEP and FRI value is the same -- the hash changes
                         commitments, not arithmetic -- and the roots, the opened paths and the nonce are the helper's;
the column-sharded LDE commitment over 2 ranks against the single-device root, and distributed.prove_sharded(hash="blake3_256") over
the same 2 ranks against prove_phases; the C++ mirror's Hash::Blake3_256 against the Python mirror and the helper."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref
from tests import backends, blake3_ref as b3, coin_ref
from tests.test_blake2s import _row_bytes
from tests.test_blake2s_prover import _splitmix
from tests.test_blake3 import _verify
from tests.test_prove_transcript import BITS, BLOWUP, FOLDING, MAXREM, NQ, SEED, setup
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3, STARK252_FP as F252, GpuVec, Matrix, MerkleTree, grind_proof_of_work, pipeline
from ministark_amd.api import F252_P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASH = "blake3_256"
WORDS = {FP: 1, GOLDILOCKS_FQ3: 3, F252: 4}
LOG_T = 10
KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = [pytest.param(FP, id="goldilocks"), pytest.param(F252, id="fp252")]


def _leaves(field, cols):
    cols = [np.asarray(c) for c in cols]
    n = len(cols[0]) // WORDS[field]
    raw = np.frombuffer(b"".join(_row_bytes(field, cols, n)), dtype=np.uint8).reshape(n, -1)
    return b3.blake3_many(raw)


def _matrix_root(field, cols):
    return b3.merkle_nodes(_leaves(field, cols))[1].tobytes()


def _layer_root(field, layer):
    rows = layer.to_numpy().reshape(-1, FOLDING, WORDS[field])
    return _matrix_root(field, [np.ascontiguousarray(rows[:, k, :]).ravel() for k in range(FOLDING)])


def _replay(out, field):
    """the verifier's side of the transcript with the helper's coin -> every draw, as canonical integers"""
    rf = coin_ref.FP252 if field == F252 else coin_ref.FP
    ints = lambda words: pipeline.from_mont_words(field, words)              # noqa: E731
    mont = lambda values: pipeline.to_mont_words(field, values).ravel()      # noqa: E731
    c = b3.Coin(SEED)
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


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", KINDS)
def test_prove(kind, field):
    pl, trace, comp, ce, nch, hints = setup(kind, field, LOG_T)
    out = pipeline.prove(pl, trace, comp, nch, hints, SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash=HASH, ce_blowup=ce, field=field, keep=True)
    mats = lambda k: [c.to_numpy() for c in out[k].columns]                  # noqa: E731
    # roots, from the downloaded values
    assert out["base_root"] == _matrix_root(field, mats("lde"))
    assert out["composition_root"] == _matrix_root(field, mats("comp_lde"))
    assert len(out["fri_roots"]) == pipeline.fri_num_layers((1 << LOG_T) * BLOWUP, BLOWUP, FOLDING, MAXREM) >= 1
    for layer, root in zip(out["fri_layers"], out["fri_roots"]):
        assert root == _layer_root(field, layer)
    # every coin draw and the proof-of-work, from the host replay
    got = _replay(out, field)
    assert out["challenges"] == got["challenges"] and out["z"] == got["z"]
    assert (out["deep"].execution_trace, out["deep"].composition_trace, out["deep"].degree) == got["deep"]
    assert out["fri_alphas"] == got["fri_alphas"]
    assert out["nonce"] == got["nonce"]
    assert out["positions"] == got["positions"] and 1 <= len(got["positions"]) <= NQ
    # openings lead to the roots
    q = out["queries"]
    assert _verify(out["base_root"], q.base_trace_proof, out["positions"])
    assert _verify(out["composition_root"], q.composition_trace_proof, out["positions"])
    for opening, root in zip(out["fri_openings"], out["fri_roots"]):
        assert _verify(root, opening["proof"], opening["positions"])


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", KINDS)
def test_prove_phases_changes_commitments_not_arithmetic(kind, field):
    pl, trace, comp, ce, nch, _ = setup(kind, field, LOG_T)
    n_lde = (1 << LOG_T) * BLOWUP
    nlayers = pipeline.fri_num_layers(n_lde, BLOWUP, FOLDING, MAXREM)
    draws = pipeline.Draws(0xB3, 8, nch, ce, NQ, n_lde, nlayers, modulus=F252_P if field == F252 else cref.GL_P)
    out = {h: pipeline.prove_phases(pl, trace, comp, draws, BLOWUP, FOLDING, MAXREM, BITS, hash=h, keep=True, ce_blowup=ce, field=field)
           for h in ("sha256", HASH)}
    s, b = out["sha256"], out[HASH]
    mats = lambda o, k: [c.to_numpy() for c in o[k].columns]                      # noqa: E731
    # every output that is not a digest is the same
    for k in ("base_polys", "lde", "comp_polys", "comp_lde", "deep_lde"):
        assert all(np.array_equal(x, y) for x, y in zip(mats(s, k), mats(b, k))), k
    assert np.array_equal(s["comp_evals"].to_numpy(), b["comp_evals"].to_numpy())
    assert len(b["fri_layers"]) == nlayers and all(np.array_equal(x.to_numpy(), y.to_numpy()) for x, y in zip(s["fri_layers"], b["fri_layers"]))
    assert np.array_equal(s["remainder"].to_numpy(), b["remainder"].to_numpy())
    assert np.array_equal(s["remainder_coeffs"], b["remainder_coeffs"])
    assert ([int(v) for v in s["ood"][0]], [int(v) for v in s["ood"][1]]) == ([int(v) for v in b["ood"][0]], [int(v) for v in b["ood"][1]])
    for k in ("base_trace_values", "composition_trace_values"):
        assert np.array_equal(getattr(s["queries"], k), getattr(b["queries"], k)), k
    assert [o["positions"] for o in s["fri_openings"]] == [o["positions"] for o in b["fri_openings"]]
    assert all(np.array_equal(x["rows"], y["rows"]) for x, y in zip(s["fri_openings"], b["fri_openings"]))
    # the digests differ, and each BLAKE3 root is the helper's over the downloaded values
    assert s["base_root"] != b["base_root"] and s["fri_roots"] != b["fri_roots"]
    assert b["base_root"] == _matrix_root(field, mats(b, "lde"))
    assert b["composition_root"] == _matrix_root(field, mats(b, "comp_lde"))
    for layer, root in zip(b["fri_layers"], b["fri_roots"]):
        assert root == _layer_root(field, layer)
    # the opened paths lead to those roots
    pos = sorted(set(draws.positions))
    q = b["queries"]
    assert _verify(b["base_root"], q.base_trace_proof, pos) and _verify(b["composition_root"], q.composition_trace_proof, pos)
    for opening, root in zip(b["fri_openings"], b["fri_roots"]):
        assert _verify(root, opening["proof"], opening["positions"])
    assert q.base_trace_proof == MerkleTree.from_matrix(b["lde"], HASH).prove(pos)
    # the nonce: the helper's search from the last FRI root
    assert b["nonce"] == b3.pow_search(b["fri_roots"][-1], BITS)


def test_names_in_the_prover():
    assert pipeline.pow_hash(HASH) == HASH and pipeline.pow_hash("blake2s") == "blake2s" and pipeline.pow_hash("poseidon252") == "sha256"
    pl, trace, comp, ce, nch, hints = setup("emu", FP, 4)
    with pytest.raises(ValueError, match="unknown"):
        pipeline.prove(pl, trace, comp, nch, hints, SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash="blake3", ce_blowup=ce)


def test_sharded_blake3_commit_and_proof_match_single_device_gloo(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dist_blake3_worker import PROVE, SHAPES, prove_inputs
    world = 2
    port = str(29800 + (os.getpid() % 400))
    procs, files = [], []
    for r in range(world):
        f = str(tmp_path / f"r{r}.txt")
        files.append(f)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_blake3_worker.py"), str(r), str(world), port, f],
                                      cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=300)
        assert p.returncode == 0, out.decode()[-2000:]
    pl = backends.planner("emu")
    want = []
    for name, V, total_cols, log_n, log_b in SHAPES:
        field = GOLDILOCKS_FQ3 if name == "fq3" else FP
        cols = [cref.lde(cref.random_elements((1 << log_n) * V, 3000 + c), log_n, log_b, V, 7, True) for c in range(total_cols)]
        root = MerkleTree.from_matrix(Matrix.from_numpy(pl, cols, field), HASH).root()
        assert root == _matrix_root(field, cols)
        want.append(root.hex())
    # prove_sharded: the base root is the helper's over the single-device LDE, the nonce a host search from the last FRI root
    log_rows, ncols, blowup, folding, max_rem, bits, _ = PROVE
    cols, comp, ce, draws = prove_inputs()
    one = pipeline.prove_phases(pl, Matrix.from_numpy(pl, cols, FP), comp, draws, blowup, folding, max_rem, bits, hash=HASH, ce_blowup=ce, keep=True)
    assert one["base_root"] == _matrix_root(FP, [c.to_numpy() for c in one["lde"].columns])
    assert one["nonce"] == b3.pow_search(one["fri_roots"][-1], bits)
    want.append(f"prove:ok:{one['base_root'].hex()}:{one['fri_roots'][-1].hex()}")
    for f in files:
        assert open(f).read().split("\n") == want


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------------

SRC = os.path.join(ROOT, "tests", "cpp", "test_blake3_mirror.cpp")


def _binary(kind):
    if kind == "emu":
        sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
        import build_emu
        so, exe, extra = build_emu.build(), os.path.join(ROOT, "tests", "cpp", "_build", "test_blake3_mirror_emu"), []
    else:
        from ministark_amd import build
        so, exe = build.build(verbose=False), os.path.join(ROOT, "tests", "cpp", "_build", "test_blake3_mirror")
        extra = ["-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)] + extra)
    return exe


def _elements(field, n, seed):
    """the C++ test's inputs: splitmix64 words below the Goldilocks prime; Fp252: the top limb cut to 59 bits"""
    w = _splitmix(n * WORDS[field], seed)
    if field == F252:
        w[3::4] >>= np.uint64(5)
    return w


MATRIX_CASES = (("fp_1x256", FP, 256, 1, 11), ("fp_17x256", FP, 256, 17, 21), ("fq3_43x64", GOLDILOCKS_FQ3, 64, 43, 41), ("fp252_97x32", F252, 32, 97, 61))
POW_SEED = bytes((i * 13 + 1) & 0xFF for i in range(32))


def _python_cases(pl):
    from ministark_amd.coin import PublicCoin
    out = []
    for name, field, n, ncols, seed in MATRIX_CASES:
        m = Matrix.from_numpy(pl, [_elements(field, n, seed + c) for c in range(ncols)], field)
        out.append({"case": name, "root": MerkleTree.from_matrix(m, HASH).root().hex()})
    ev = GpuVec.from_numpy(pl, _splitmix(1 << 10, 51), FP)
    out.append({"case": "fri_fp_8", "root": MerkleTree.from_fri_layer(ev, 8, HASH).root().hex()})
    coin = PublicCoin(pl, POW_SEED, HASH)
    coin.reseed_int(5)
    out.append({"case": "pow", "nonce": grind_proof_of_work(pl, POW_SEED, 9, hash=HASH), "sha256": grind_proof_of_work(pl, POW_SEED, 9),
                "coin_nonce": coin.grind(9), "coin_word": int(coin.draw(FP, 1).to_numpy()[0])})
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_cpp_mirror_matches_python_and_the_helper(kind, tmp_path):
    exe = _binary(kind)
    # the helper's digests go to the program through a file under the test's temporary directory: it compares every root itself
    want = {name: _matrix_root(field, [_elements(field, n, seed + c) for c in range(ncols)]).hex() for name, field, n, ncols, seed in MATRIX_CASES}
    rows = _splitmix(1 << 10, 51).reshape(-1, 8)
    want["fri_fp_8"] = _matrix_root(FP, [np.ascontiguousarray(rows[:, k]) for k in range(8)]).hex()
    path = tmp_path / "blake3_digests.txt"
    path.write_text("".join(f"{name} {root}\n" for name, root in want.items()))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "cpp blake3 mirror ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    cpp = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    assert {c["case"]: c["root"] for c in cpp if "root" in c} == want
    assert cpp == _python_cases(backends.planner(kind))
    # a wrong digest in the file makes the program fail
    path.write_text("".join(f"{name} {root if name != 'fq3_43x64' else root[::-1]}\n" for name, root in want.items()))
    bad = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 1 and "fq3_43x64" in bad.stderr and "cpp blake3 mirror ok" not in bad.stdout
    # and the helper's coin: reseed_int(5), grind 9 bits, one Goldilocks draw
    case = [c for c in cpp if c["case"] == "pow"][0]
    ref = b3.Coin(POW_SEED)
    assert case["nonce"] == ref.grind(9)
    ref.reseed_int(5)
    assert case["coin_nonce"] == ref.grind(9) and [case["coin_word"]] == ref.draw(coin_ref.FP, 1)
