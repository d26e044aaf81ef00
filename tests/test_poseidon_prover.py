"""prove_phases and prove over the 252-bit field with hash="poseidon252" (fib AIR, 8 columns, offset 3): what they return is checked the
way tests/test_fp252_prover.py checks the byte hashes, in Python integers -- on the small size the committed roots are recomputed from
the downloaded rows with tests/poseidon_ref.py; at both sizes the out-of-domain consistency of the composition, the DEEP value at every
query from the opened rows, each FRI layer's fold at the queried cosets, the remainder, and the proof-of-work nonce, which a Poseidon
prover grinds with SHA-256 over the last root's 32 bytes."""
import hashlib

import numpy as np
import pytest

from tests import backends, poseidon_ref as ref
from tests.test_fp252_prover import BITS, BLOWUP, NQ, _eval_at, _fib_trace, _lz, _rev, _value, _values
from tests.test_prove_transcript import FOLDING, MAXREM, SEED, ReplayedDraws, replay, same, setup
from ministark_amd import GOLDILOCKS_FP, STARK252_FP as F, Matrix, Radix2EvaluationDomain, pipeline, poseidon252_value
from ministark_amd.api import F252_P as p, f252_to_mont_limbs

HASH = "poseidon252"
CASES = [pytest.param(kind, log_t, folding, id=f"{kind}-2^{log_t}-fold{folding}", marks=[pytest.mark.gpu] if kind == "hip" else [])
         for kind, log_t in (("emu", 8), ("hip", 16)) for folding in (8, 4)]


def _root(rows):
    """rows: lists of canonical integers; a leaf is hash_many(row), a node hash2(left, right) -> the root's integer"""
    return ref.merkle_nodes([ref.hash_many(r) for r in rows])[1]


@pytest.mark.parametrize("kind,log_t,folding", CASES)
def test_proof_over_the_252_bit_field_with_poseidon(kind, log_t, folding):
    pl = backends.planner(kind)
    n = 1 << log_t
    N = n * BLOWUP
    cols = _fib_trace(n)
    trace = Matrix.from_numpy(pl, [np.concatenate([f252_to_mont_limbs(v) for v in c]).astype(np.uint64) for c in cols], F)
    comp, ce, nch = pipeline.fib_constraints(n, 8, F)
    nlayers = pipeline.fri_num_layers(N, BLOWUP, folding, 64)
    draws = pipeline.Draws(252 + folding, 8, nch, ce, NQ, N, nlayers, modulus=p)
    draws.hints = [cols[7][n - 1]]
    out = pipeline.prove_phases(pl, trace, comp, draws, BLOWUP, folding, 64, BITS, hash=HASH, keep=True, ce_blowup=ce, field=F)
    assert len(out["fri_roots"]) == nlayers >= 1
    # (a) the roots, from the downloaded rows (the small size only)
    if kind == "emu":
        for key, root in (("lde", out["base_root"]), ("comp_lde", out["composition_root"])):
            cs = [_values(c) for c in out[key].to_numpy()]
            assert poseidon252_value(root) == _root([list(r) for r in zip(*cs)]), key
        for layer, root in zip(out["fri_layers"], out["fri_roots"]):
            v = _values(layer.to_numpy())
            assert poseidon252_value(root) == _root([v[i:i + folding] for i in range(0, len(v), folding)])
    # (c) the nonce: SHA-256 over the last root's 32 bytes as they lie in memory, the smallest nonce from 1 with BITS leading zero bits
    nonce = 1
    while _lz(hashlib.sha256(out["fri_roots"][-1] + nonce.to_bytes(8, "big")).digest()) < BITS:
        nonce += 1
    assert out["nonce"] == nonce
    # (b) 1. out-of-domain consistency of the composition (ce = 1: one composition column, its point z^1 = z)
    args, z = draws.trace_args, draws.z
    execution, composition = [int(v) for v in out["ood"][0]], [int(v) for v in out["ood"][1]]
    assert ce == 1 and len(composition) == 1
    assert _eval_at(comp, z, dict(zip(args, execution)), draws.challenges, draws.hints) == composition[0]
    # (b) 2. the DEEP value at every query, from the opened trace and composition rows
    q, coeffs = out["queries"], draws.deep
    g = Radix2EvaluationDomain(n, 1, F).group_gen
    w = Radix2EvaluationDomain(N, 1, F).group_gen
    log_N = N.bit_length() - 1
    layer0 = out["deep_lde"].columns[0].to_numpy().reshape(-1, 4)
    for i, pos in enumerate(draws.positions):
        x = 3 * pow(w, _rev(pos, log_N), p) % p
        acc = 0
        for j, ((col, off), ood) in enumerate(zip(args, execution)):
            acc += coeffs.execution_trace[j] * (_value(q.base_trace_values[i][4 * col:4 * col + 4]) - ood) * pow((x - z * pow(g, off, p)) % p, -1, p)
        acc += coeffs.composition_trace[0] * (_value(q.composition_trace_values[i][:4]) - composition[0]) * pow((x - z) % p, -1, p)
        assert _value(layer0[pos]) == acc % p * ((coeffs.degree[0] + coeffs.degree[1] * x) % p) % p, f"query {i} at position {pos}"
    # (b) 3. every FRI layer's fold at the queried cosets (the FRI domain is taken without its offset), then the remainder
    log_f = folding.bit_length() - 1
    wf = Radix2EvaluationDomain(folding, 1, F).group_gen
    positions = sorted(set(draws.positions))
    evaluations = [_value(layer0[pos]) for pos in positions]
    gen, size = w, N
    assert len(out["fri_openings"]) == nlayers
    for opening, alpha in zip(out["fri_openings"], draws.fri_alphas):
        folded = pipeline.fold_positions(positions, folding)
        assert opening["positions"] == folded
        rows = [_values(row) for row in opening["rows"]]
        assert [rows[folded.index(pos // folding)][pos % folding] for pos in positions] == evaluations
        nxt = []
        for row, fp in zip(rows, folded):
            offset = pow(gen, _rev(fp, (size // folding).bit_length() - 1), p)
            vals = [row[_rev(k, log_f)] for k in range(folding)]
            cs = [sum(v * pow(offset * pow(wf, k, p) % p, -j, p) for k, v in enumerate(vals)) % p for j in range(folding)]
            nxt.append(sum(c * pow(alpha, j, p) for j, c in enumerate(cs)) % p)
        evaluations, positions, gen, size = nxt, folded, pow(gen, folding, p), size // folding
    rem = _values(out["remainder_coeffs"])
    assert len(rem) == max(size // BLOWUP, 1)
    full = _values(out["remainder"].to_numpy())
    assert len(full) == size
    pts = range(size) if kind == "emu" else positions
    for pos in pts:
        x = pow(gen, _rev(pos, size.bit_length() - 1), p)
        assert sum(c * pow(x, j, p) for j, c in enumerate(rem)) % p == full[pos]
    for pos, want in zip(positions, evaluations):
        assert full[pos] == want
    # the openings lead to the committed roots (the small size: hash2 in Python integers)
    if kind == "emu":
        from tests.test_poseidon252 import _verify
        assert _verify(poseidon252_value(out["base_root"]), q.base_trace_proof, draws.positions)
        assert _verify(poseidon252_value(out["composition_root"]), q.composition_trace_proof, draws.positions)
        for opening, root in zip(out["fri_openings"], out["fri_roots"]):
            assert _verify(poseidon252_value(root), opening["proof"], opening["positions"])


@pytest.mark.parametrize("kind,log_t", [pytest.param("emu", 7, id="emu"), pytest.param("hip", 10, id="hip", marks=pytest.mark.gpu)])
def test_prove_gives_the_roots_of_prove_phases_fed_the_coins_draws(kind, log_t):
    """pipeline.prove draws from the SHA-256 byte coin over the roots' 32 bytes; the verifier's replay of that transcript reproduces
    every draw, and prove_phases fed those draws commits to the same roots and opens the same proofs"""
    pl, trace, comp, ce, nch, hints = setup(kind, F, log_t)
    out = pipeline.prove(pl, trace, comp, nch, hints, SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash=HASH, ce_blowup=ce, field=F)
    got = replay(out, F, "sha256")
    assert out["challenges"] == got["challenges"] and out["z"] == got["z"] and out["fri_alphas"] == got["fri_alphas"]
    assert out["nonce"] == got["nonce"] and out["positions"] == got["positions"]
    phases = pipeline.prove_phases(pl, trace, comp, ReplayedDraws(got, hints, out["trace_args"]), BLOWUP, FOLDING, MAXREM, BITS, hash=HASH,
                                   ce_blowup=ce, time_phases=False, field=F)
    for key in ("base_root", "composition_root", "fri_roots", "ood"):
        assert same(out[key], phases[key]), key
    assert same(out["fri_openings"], phases["fri_openings"])
    assert same(out["queries"].base_trace_proof, phases["queries"].base_trace_proof)
    other = pipeline.prove(pl, trace, comp, nch, hints, SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash="sha256", ce_blowup=ce, field=F)
    assert other["base_root"] != out["base_root"]


def test_goldilocks_with_poseidon_is_refused_and_rpo_names_the_alternative():
    pl, trace, comp, ce, nch, hints = setup("emu", GOLDILOCKS_FP, 4)
    draws = pipeline.Draws(1, 8, nch, ce, 4, 16 * BLOWUP, 1)
    with pytest.raises(ValueError, match="poseidon252 absorbs elements of the 252-bit field"):
        pipeline.prove_phases(pl, trace, comp, draws, BLOWUP, 8, 64, BITS, hash=HASH, ce_blowup=ce)
    with pytest.raises(ValueError, match="poseidon252 absorbs elements of the 252-bit field"):
        pipeline.prove(pl, trace, comp, nch, hints, SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash=HASH, ce_blowup=ce)
    pl, trace, comp, ce, nch, hints = setup("emu", F, 4)
    draws = pipeline.Draws(1, 8, nch, ce, 4, 16 * BLOWUP, 1, modulus=p)
    with pytest.raises(ValueError, match="RPO-256 absorbs Goldilocks elements.*poseidon252"):
        pipeline.prove_phases(pl, trace, comp, draws, BLOWUP, 8, 64, BITS, hash="rpo256", ce_blowup=ce, field=F)
    with pytest.raises(ValueError, match="RPO-256 absorbs Goldilocks elements.*poseidon252"):
        pipeline.prove(pl, trace, comp, nch, hints, SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash="rpo256", ce_blowup=ce, field=F)
    assert pipeline.pow_hash(HASH) == "sha256"


def test_default_arguments_still_give_the_recorded_goldilocks_proof():
    """prove_phases with default arguments (Goldilocks, SHA-256) on the simulator: roots, nonce and remainder as recorded in
    tests/golden/prove_phases_default_emu_2_8.json"""
    import json
    import os
    from oracle import cref
    want = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "prove_phases_default_emu_2_8.json")))
    pl = backends.planner("emu")
    n_t, ncols, seed = 1 << 8, 8, 4242
    cols = [cref.random_elements(n_t, seed + c) for c in range(ncols)]
    comp, ce, nch = pipeline.fib_constraints(n_t, ncols)
    draws = pipeline.Draws(seed, ncols, nch, ce, 32, n_t * 4, pipeline.fri_num_layers(n_t * 4, 4, 8, 64))
    out = pipeline.prove_phases(pl, Matrix.from_numpy(pl, cols, GOLDILOCKS_FP), comp, draws, ce_blowup=ce)
    got = {"base_root": bytes(out["base_root"]).hex(), "composition_root": bytes(out["composition_root"]).hex(),
           "fri_roots": [bytes(r).hex() for r in out["fri_roots"]], "nonce": int(out["nonce"]),
           "remainder": [int(v) for v in out["remainder"].to_numpy()], "remainder_coeffs": [int(v) for v in out["remainder_coeffs"]]}
    assert got == want
