"""`pipeline.prove` -- the prover's phases with every challenge drawn from the device-resident public coin -- on the fib AIR, over
Goldilocks and the 252-bit field, with SHA-256 and BLAKE2s:
  (a) tests/coin_ref.py replays the transcript from what the proof itself carries (roots, out-of-domain values, remainder, nonce) and
      must arrive at every draw the prover reports: composition coefficients, z, DEEP coefficients, FRI alphas, query positions;
  (b) `pipeline.prove_phases`, handed those replayed values as its fixed draws, returns the same commitments, FRI roots, remainder,
      out-of-domain values and openings (its nonce is not compared with prove's: it grinds on the last FRI root by design; prove's nonce
      is compared with coin_ref's search on the replayed seed);
  (c) one changed byte of the seed changes z."""
import numpy as np
import pytest

from tests import backends, coin_ref
from tests.test_verifier_relations import fib_trace
from ministark_amd import GOLDILOCKS_FP, STARK252_FP, Matrix, pipeline
from ministark_amd.api import F252_P, f252_to_mont_limbs, gl_to_mont
from ministark_amd.composer import DeepCompositionCoeffs

BLOWUP, FOLDING, MAXREM, BITS, NQ = 4, 8, 64, 8, 32
SEED = bytes(range(7, 39))
CASES = [pytest.param(kind, field, log_t, hash, id=f"{kind}-{name}-{hash}", marks=[pytest.mark.gpu] if kind == "hip" else [])
         for kind, sizes in (("emu", {GOLDILOCKS_FP: 8, STARK252_FP: 7}), ("hip", {GOLDILOCKS_FP: 12, STARK252_FP: 10}))
         for field, name in ((GOLDILOCKS_FP, "goldilocks"), (STARK252_FP, "fp252")) for log_t in (sizes[field],)
         for hash in ("sha256", "blake2s")]
_proofs = {}


def fib_trace_252(n):
    cols, v = [[0] * n for _ in range(8)], [1, 2]
    for k in range(2, 8):
        v.append(v[k - 2] * v[k - 1] % F252_P)
    for r in range(n):
        for k in range(8):
            cols[k][r] = v[k]
        w = [v[6] * v[7] % F252_P]
        w.append(v[7] * w[0] % F252_P)
        for k in range(2, 8):
            w.append(w[k - 2] * w[k - 1] % F252_P)
        v = w
    return cols


def setup(kind, field, log_t):
    pl, n = backends.planner(kind), 1 << log_t
    if field == STARK252_FP:
        cols = fib_trace_252(n)
        trace = Matrix.from_numpy(pl, [np.concatenate([f252_to_mont_limbs(v) for v in c]).astype(np.uint64) for c in cols], field)
    else:
        cols = fib_trace(n)
        trace = Matrix.from_numpy(pl, [np.array([gl_to_mont(v) for v in c], dtype=np.uint64) for c in cols], field)
    comp, ce, nch = pipeline.fib_constraints(n, 8, field)
    return pl, trace, comp, ce, nch, [cols[7][n - 1]]


def run(kind, field, log_t, hash, seed=SEED):
    pl, trace, comp, ce, nch, hints = setup(kind, field, log_t)
    return pipeline.prove(pl, trace, comp, nch, hints, seed, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash=hash, ce_blowup=ce, field=field)


def proof(kind, field, log_t, hash):
    """one proof per case, shared by the tests and left unchanged"""
    key = (kind, field, log_t, hash)
    if key not in _proofs:
        _proofs[key] = run(*key)
    return _proofs[key]


def replay(out, field, hash):
    """the verifier's side of the transcript, from the proof's own contents -> every draw, as canonical integers"""
    rf = coin_ref.FP252 if field == STARK252_FP else coin_ref.FP
    ints = lambda words: pipeline.from_mont_words(field, words)
    mont = lambda values: pipeline.to_mont_words(field, values).ravel()
    c = coin_ref.Coin(SEED, hash)
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


@pytest.mark.parametrize("kind,field,log_t,hash", CASES)
def test_the_replayed_transcript_reproduces_every_draw(kind, field, log_t, hash):
    out = proof(kind, field, log_t, hash)
    got = replay(out, field, hash)
    assert len(out["fri_roots"]) == pipeline.fri_num_layers((1 << log_t) * BLOWUP, BLOWUP, FOLDING, MAXREM) >= 1
    assert out["challenges"] == got["challenges"]
    assert out["z"] == got["z"]
    assert (out["deep"].execution_trace, out["deep"].composition_trace, out["deep"].degree) == got["deep"]
    assert out["fri_alphas"] == got["fri_alphas"]
    assert out["nonce"] == got["nonce"]
    assert out["positions"] == got["positions"] and 1 <= len(got["positions"]) <= NQ


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


class ReplayedDraws:
    """what `pipeline.Draws` carries, filled from the replayed transcript"""
    def __init__(self, got, hints, trace_args):
        self.challenges, self.hints, self.z, self.trace_args = got["challenges"], hints, got["z"], trace_args
        self.deep = DeepCompositionCoeffs(*got["deep"])
        self.fri_alphas, self.positions = got["fri_alphas"], got["positions"]


@pytest.mark.parametrize("kind,field,log_t,hash", CASES)
def test_prove_phases_with_the_replayed_draws_gives_the_same_proof(kind, field, log_t, hash):
    out = proof(kind, field, log_t, hash)
    pl, trace, comp, ce, nch, hints = setup(kind, field, log_t)
    draws = ReplayedDraws(replay(out, field, hash), hints, out["trace_args"])
    ref = pipeline.prove_phases(pl, trace, comp, draws, BLOWUP, FOLDING, MAXREM, BITS, hash=hash, ce_blowup=ce, time_phases=False, field=field)
    for key in ("base_root", "composition_root", "fri_roots", "ood"):
        assert same(out[key], ref[key]), key
    assert np.array_equal(out["remainder_coeffs"], ref["remainder_coeffs"])
    assert np.array_equal(out["remainder"].to_numpy(), ref["remainder"].to_numpy())
    for member in ("base_trace_proof", "composition_trace_proof", "base_trace_values", "composition_trace_values"):
        assert same(getattr(out["queries"], member), getattr(ref["queries"], member)), member
    assert same(out["fri_openings"], ref["fri_openings"])


@pytest.mark.parametrize("kind,field,log_t,hash", CASES)
def test_one_changed_seed_byte_changes_z(kind, field, log_t, hash):
    other = run(kind, field, log_t, hash, SEED[:13] + bytes([SEED[13] ^ 1]) + SEED[14:])
    assert other["z"] != proof(kind, field, log_t, hash)["z"]
