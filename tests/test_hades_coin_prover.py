"""`pipeline.prove(..., hash="poseidon252", field=STARK252_FP, coin="poseidon252")`: the whole transcript on the algebraic coin of the
252-bit field (coin.PoseidonCoin).  A host replay with tests/hades_coin_ref.py is fed only what a proof carries -- the roots, the
out-of-domain values, the remainder coefficients and the nonce -- and reproduces every draw: challenges, z, DEEP coefficients, FRI
alphas, nonce and positions; the nonce meets the condition and is the smallest.  The fib AIR at the size tests/test_poseidon_prover.py
proves.  coin=None is the byte-coin prover, word for word."""
import pytest

from tests import hades_coin_ref
from tests.test_fp252_prover import BITS, BLOWUP, NQ
from tests.test_prove_transcript import FOLDING, MAXREM, SEED, ReplayedDraws, replay as byte_replay, same, setup
from ministark_amd import GOLDILOCKS_FP, STARK252_FP as F, pipeline, poseidon252_value
from ministark_amd.api import F252_P as p

HASH = "poseidon252"
COIN_SEED = 0x0123456789abcdef0fedcba987654321aa55aa55deadbeef0011223344556677 % p
SIZES = [pytest.param("emu", 7, id="emu"), pytest.param("hip", 10, id="hip", marks=pytest.mark.gpu)]
_proofs = {}


def proof(kind, log_t):
    """one proof per backend, shared by the tests and left unchanged"""
    if kind not in _proofs:
        pl, trace, comp, ce, nch, hints = setup(kind, F, log_t)
        out = pipeline.prove(pl, trace, comp, nch, hints, COIN_SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash=HASH, ce_blowup=ce, field=F, keep=True,
                             coin=HASH)
        _proofs[kind] = (out, (pl, trace, comp, ce, nch, hints))
    return _proofs[kind]


def replay(out, seed=COIN_SEED):
    """the verifier's side of the transcript: every draw as canonical integers, from the proof's contents alone"""
    c = hades_coin_ref.Coin(seed)
    got = {}
    c.reseed_digest(poseidon252_value(out["base_root"]))
    got["challenges"] = c.draw(len(out["challenges"]))
    c.reseed_digest(poseidon252_value(out["composition_root"]))
    got["z"] = c.draw(1)[0]
    c.reseed_elements([int(v) for v in list(out["ood"][0]) + list(out["ood"][1])])
    nexec, ncomp = len(out["ood"][0]), len(out["ood"][1])
    d = c.draw(nexec + ncomp + 2)
    got["deep"] = (d[:nexec], d[nexec: nexec + ncomp], (d[-2], d[-1]))
    got["fri_alphas"] = []
    for root in out["fri_roots"]:
        c.reseed_digest(poseidon252_value(root))
        got["fri_alphas"].append(c.draw(1)[0])
    c.reseed_elements(pipeline.from_mont_words(F, out["remainder_coeffs"]))
    got["before_grind"] = c.copy()
    got["nonce"] = c.grind(BITS)
    c.reseed_int(out["nonce"])
    got["positions"] = c.draw_queries(NQ, len(out["remainder"]) * FOLDING ** len(out["fri_roots"]))
    got["permutations"], got["final"] = c.permutations, c.state()
    return got


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_the_replayed_transcript_reproduces_every_draw(kind, log_t):
    out, _ = proof(kind, log_t)
    got = replay(out)
    print(f"transcript permutations: {got['permutations']} (+ the search), nonce {out['nonce']}")
    assert len(out["fri_roots"]) == pipeline.fri_num_layers((1 << log_t) * BLOWUP, BLOWUP, FOLDING, MAXREM) >= 1
    assert out["challenges"] == got["challenges"] and out["z"] == got["z"]
    assert (out["deep"].execution_trace, out["deep"].composition_trace, out["deep"].degree) == got["deep"]
    assert out["fri_alphas"] == got["fri_alphas"] and len(got["fri_alphas"]) == len(out["fri_roots"])
    # the nonce is the smallest that meets the condition
    assert out["nonce"] == got["nonce"] >= 1
    assert got["before_grind"].accepts(out["nonce"], BITS) and not any(got["before_grind"].accepts(k, BITS) for k in range(1, out["nonce"]))
    assert out["positions"] == got["positions"] and 1 <= len(got["positions"]) <= NQ
    assert out["coin"].state() == got["final"]                                 # the device coin ends where the replay ends
    assert out["coin"].hash == HASH


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_prove_phases_fed_the_replayed_draws_commits_to_the_same_roots(kind, log_t):
    out, (pl, trace, comp, ce, nch, hints) = proof(kind, log_t)
    got = replay(out)
    phases = pipeline.prove_phases(pl, trace, comp, ReplayedDraws(got, hints, out["trace_args"]), BLOWUP, FOLDING, MAXREM, BITS, hash=HASH,
                                   ce_blowup=ce, time_phases=False, field=F)
    for key in ("base_root", "composition_root", "fri_roots", "ood"):
        assert same(out[key], phases[key]), key
    assert same(out["fri_openings"], phases["fri_openings"])
    assert same(out["queries"].base_trace_proof, phases["queries"].base_trace_proof)


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_coin_none_is_the_byte_coin_prover(kind, log_t):
    """coin=None draws from the SHA-256 byte coin over the roots' 32 bytes, as before: the byte replay reproduces it, and it is the
    proof that leaving `coin` out gives"""
    pl, trace, comp, ce, nch, hints = setup(kind, F, log_t)
    out = pipeline.prove(pl, trace, comp, nch, hints, SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash=HASH, ce_blowup=ce, field=F, coin=None)
    got = byte_replay(out, F, "sha256")
    assert out["challenges"] == got["challenges"] and out["z"] == got["z"] and out["fri_alphas"] == got["fri_alphas"]
    assert out["nonce"] == got["nonce"] and out["positions"] == got["positions"]
    default = pipeline.prove(pl, trace, comp, nch, hints, SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash=HASH, ce_blowup=ce, field=F)
    for key in ("base_root", "composition_root", "fri_roots", "ood", "nonce", "positions", "challenges", "z", "fri_alphas", "fri_openings"):
        assert same(out[key], default[key]), key
    algebraic, _ = proof(kind, log_t)
    assert same(out["base_root"], algebraic["base_root"]) and out["z"] != algebraic["z"]      # the same trace, another transcript
    assert pipeline.pow_hash(HASH) == "sha256"


def test_the_refusals():
    pl, trace, comp, ce, nch, hints = setup("emu", F, 4)
    args = (pl, trace, comp, nch, hints)
    tail = (BLOWUP, FOLDING, MAXREM, BITS, NQ)
    with pytest.raises(ValueError, match='coin="poseidon252"'):
        pipeline.prove(*args, COIN_SEED, *tail, hash="sha256", ce_blowup=ce, field=F, coin=HASH)                # another hash
    with pytest.raises(ValueError, match="coin is None"):
        pipeline.prove(*args, COIN_SEED, *tail, hash=HASH, ce_blowup=ce, field=F, coin="keccak256")
    with pytest.raises(ValueError, match="below p"):
        pipeline.prove(*args, SEED, *tail, hash=HASH, ce_blowup=ce, field=F, coin=HASH)                          # 32 bytes that read as an integer >= p
    with pytest.raises(ValueError, match="below p"):
        pipeline.prove(*args, p, *tail, hash=HASH, ce_blowup=ce, field=F, coin=HASH)
    with pytest.raises(ValueError, match='coin="rpo256"'):
        pipeline.prove(*args, [1, 2, 3, 4], *tail, hash=HASH, ce_blowup=ce, field=F, coin="rpo256")               # the other algebraic coin, the wrong field
    gpl, gtrace, gcomp, gce, gnch, ghints = setup("emu", GOLDILOCKS_FP, 4)
    with pytest.raises(ValueError, match='coin="poseidon252"'):
        pipeline.prove(gpl, gtrace, gcomp, gnch, ghints, COIN_SEED, *tail, hash="rpo256", ce_blowup=gce, coin=HASH)   # another field
    with pytest.raises(ValueError, match="poseidon252 absorbs elements of the 252-bit field"):
        pipeline.prove(gpl, gtrace, gcomp, gnch, ghints, COIN_SEED, *tail, hash=HASH, ce_blowup=gce, coin=HASH)       # the older refusal keeps its message
