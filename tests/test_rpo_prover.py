"""`pipeline.prove(..., hash="rpo256", coin="rpo256")`: the whole transcript on the algebraic coin (coin.RpoCoin).  A host replay with
tests/rpo_coin_ref.py is fed only what a proof carries -- the roots, the out-of-domain values, the remainder coefficients and the nonce --
and reproduces every draw; the nonce meets the condition and is the smallest; the openings lead to the RPO roots; and the relations of
tests/test_verifier_relations.py hold on the proof: out-of-domain consistency, the DEEP composition at the query positions, the low
degree of the remainder, the FRI openings folding into each other and into the remainder.  The fib AIR at 2^6 rows x 8 columns with
folding 8 and folding 2, and `lookup_air` over Fq3.  coin=None is today's prover, word for word."""
from collections import deque

import numpy as np
import pytest

from oracle.pyref import rpo as pyrpo
from tests import backends, rpo_coin_ref
from tests.test_extension_prover import high_remainder_coefficients, ood_consistent
from tests.test_verifier_relations import eval_at, fib_trace
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, STARK252_FP as F252, Matrix, Radix2EvaluationDomain, pipeline
from ministark_amd.api import GL_P as P, gl_from_mont, gl_to_mont

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
LOG_T, BLOWUP, BITS, NQ = 6, 4, 6, 16
MAXREM = 4                                 # 2^8 LDE points: two layers of folding 8 (256 -> 32 -> 4), four of folding 2 (256 -> ... -> 16)
SEED = [3, 1, 4, 1 << 40]
_proofs = {}


def digest(b):
    """the 32 bytes of an RPO digest as the library stores it -> four canonical integers"""
    return [gl_from_mont(int(w)) for w in np.frombuffer(b, dtype=np.uint64)]


def canon(words):
    return [gl_from_mont(int(w)) for w in np.asarray(words).ravel()]


def flat(values):
    """canonical Fp integers or Fq3 3-tuples -> base-field words in memory order"""
    return [int(w) for v in values for w in (v if isinstance(v, tuple) else (v,))]


def fib_proof(kind, folding):
    """one proof per case, shared by the tests and left unchanged"""
    key = (kind, "fib", folding)
    if key not in _proofs:
        pl, n = backends.planner(kind), 1 << LOG_T
        cols = fib_trace(n)
        trace = Matrix.from_numpy(pl, [np.array([gl_to_mont(v) for v in c], dtype=np.uint64) for c in cols], FP)
        comp, ce, nch = pipeline.fib_constraints(n, 8)
        hints = [cols[7][n - 1]]
        out = pipeline.prove(pl, trace, comp, nch, hints, SEED, BLOWUP, folding, MAXREM, BITS, NQ, hash="rpo256", keep=True, ce_blowup=ce,
                             coin="rpo256")
        _proofs[key] = (out, comp, ce, hints)
    return _proofs[key]


def lookup_proof(kind):
    key = (kind, "lookup")
    if key not in _proofs:
        pl, n = backends.planner(kind), 1 << LOG_T
        cols = pipeline.lookup_trace(n, 70 + LOG_T)
        trace = Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols], FP)
        comp, ce, ncoef, nair, columns = pipeline.lookup_air(n)
        out = pipeline.prove(pl, trace, comp, ncoef, [], SEED, BLOWUP, 8, MAXREM, BITS, NQ, hash="rpo256", keep=True, ce_blowup=ce, fq=FQ3F,
                             num_air_challenges=nair, extension=columns, coin="rpo256")
        _proofs[key] = (out, comp, nair)
    return _proofs[key]


def replay(out, nair, V, folding, seed=SEED):
    """the verifier's side of the transcript: every draw as canonical values (3-tuples when V = 3), from the proof's contents alone"""
    vals = lambda words: [tuple(words[k:k + 3]) for k in range(0, len(words), 3)] if V == 3 else list(words)
    c = rpo_coin_ref.Coin(seed)
    got = {}
    c.reseed_digest(digest(out["base_root"]))
    got["air_challenges"] = vals(c.draw(V * nair))
    if "extension_root" in out:
        c.reseed_digest(digest(out["extension_root"]))
    got["challenges"] = vals(c.draw(V * len(out["challenges"])))
    c.reseed_digest(digest(out["composition_root"]))
    got["z"] = vals(c.draw(V))[0]
    c.reseed_elements(flat(list(out["ood"][0]) + list(out["ood"][1])))
    nexec, ncomp = len(out["ood"][0]), len(out["ood"][1])
    d = vals(c.draw(V * (nexec + ncomp + 2)))
    got["deep"] = (d[:nexec], d[nexec: nexec + ncomp], (d[-2], d[-1]))
    got["fri_alphas"] = []
    for root in out["fri_roots"]:
        c.reseed_digest(digest(root))
        got["fri_alphas"].append(vals(c.draw(V))[0])
    c.reseed_elements(canon(out["remainder_coeffs"]))
    got["before_grind"] = c.copy()
    got["nonce"] = c.grind(BITS)
    c.reseed_int(out["nonce"])
    got["after_nonce"] = c.copy()
    got["positions"] = c.draw_queries(NQ, len(out["remainder"]) * folding ** len(out["fri_roots"]))
    got["permutations"], got["final"] = c.permutations, c.state()
    return got


def check_replay(out, nair, V, folding):
    got = replay(out, nair, V, folding)
    print(f"transcript permutations: {got['permutations']} (+ the search), nonce {out['nonce']}")
    assert len(out["fri_roots"]) == pipeline.fri_num_layers((1 << LOG_T) * BLOWUP, BLOWUP, folding, MAXREM) >= 2
    assert out["air_challenges"] == got["air_challenges"] and len(got["air_challenges"]) == nair
    assert out["challenges"] == got["challenges"] and out["z"] == got["z"]
    assert (out["deep"].execution_trace, out["deep"].composition_trace, out["deep"].degree) == got["deep"]
    assert out["fri_alphas"] == got["fri_alphas"] and len(got["fri_alphas"]) == len(out["fri_roots"])
    # the nonce is the smallest that meets the condition, and the state after absorbing it shows the zero bits in a capacity element
    assert out["nonce"] == got["nonce"] >= 1
    assert got["before_grind"].accepts(out["nonce"], BITS) and not any(got["before_grind"].accepts(k, BITS) for k in range(1, out["nonce"]))
    assert got["after_nonce"].s[0] & ((1 << BITS) - 1) == 0
    assert out["positions"] == got["positions"] and 1 <= len(got["positions"]) <= NQ
    assert out["coin"].state() == got["final"]                                 # the device coin ends where the replay ends
    return got


def verify_opening(root, view, indices):
    """MerkleTreeImpl::verify (src/merkle.rs:208-287) with the RPO-256 merge: True iff the batched opening leads to `root`"""
    h = lambda l, r: pyrpo.merge(l, r)
    n = 1 << view["height"]
    siblings, nodes = deque(digest(b) for b in view["sibling_leaves"]), deque(digest(b) for b in view["nodes"])
    leaves = deque(zip(sorted(set(indices)), [digest(b) for b in view["initial_leaves"]]))
    queue = deque()
    while leaves:
        i, leaf = leaves.popleft()
        if leaves and (i ^ 1) == leaves[0][0]:
            queue.append(((n + i) >> 1, h(leaf, leaves.popleft()[1])))
            continue
        s = siblings.popleft()
        queue.append(((n + i) >> 1, h(leaf, s) if i % 2 == 0 else h(s, leaf)))
    while queue:
        i, d = queue.popleft()
        if i == 1:
            return d == digest(root) and not siblings and not nodes
        if queue and (i ^ 1) == queue[0][0]:
            queue.append((i >> 1, h(d, queue.popleft()[1])))
            continue
        s = nodes.popleft()
        queue.append((i >> 1, h(d, s) if i % 2 == 0 else h(s, d)))
    return False


def check_openings(out, folding):
    """verify_rows (src/merkle.rs:208-293): the opened rows hash to the opening's leaves, which lead to the committed roots"""
    q, positions = out["queries"], out["positions"]
    opened = [(q.base_trace_values, q.base_trace_proof, out["base_root"]), (q.composition_trace_values, q.composition_trace_proof, out["composition_root"])]
    if "extension_root" in out:
        opened.append((q.extension_trace_values, q.extension_trace_proof, out["extension_root"]))
    for rows, proof, root in opened:
        assert [pyrpo.hash_row(canon(r)) for r in rows] == [digest(b) for b in proof["initial_leaves"]]
        assert verify_opening(root, proof, positions)
    pos = positions
    for opening, root in zip(out["fri_openings"], out["fri_roots"]):
        pos = pipeline.fold_positions(pos, folding)
        assert opening["positions"] == pos
        assert [pyrpo.hash_row(canon(r)) for r in opening["rows"]] == [digest(b) for b in opening["proof"]["initial_leaves"]]
        assert verify_opening(root, opening["proof"], pos)
        bad = dict(opening["proof"], initial_leaves=[bytes(32)] + list(opening["proof"]["initial_leaves"])[1:])
        assert not verify_opening(root, bad, pos)


@pytest.mark.parametrize("folding", [8, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_a_host_replay_reproduces_every_draw_and_the_openings_verify(kind, folding):
    out, _, _, _ = fib_proof(kind, folding)
    check_replay(out, 0, 1, folding)
    check_openings(out, folding)


@pytest.mark.parametrize("folding", [8, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_the_verifier_relations_hold_on_the_proof(kind, folding):
    out, comp, ce, hints = fib_proof(kind, folding)
    n, N = 1 << LOG_T, (1 << LOG_T) * BLOWUP
    log_N, log_f = N.bit_length() - 1, folding.bit_length() - 1
    rev = lambda v, bits: int(format(v, f"0{bits}b")[::-1], 2) if bits else 0
    execution, composition = [int(v) for v in out["ood"][0]], [int(v) for v in out["ood"][1]]
    z, deep, positions, q = out["z"], out["deep"], out["positions"], out["queries"]
    # 1. out-of-domain consistency (src/verifier.rs:82-95)
    trace_at = dict(zip(out["trace_args"], execution))
    provided = sum(h * pow(z, k, P) for k, h in enumerate(composition)) % P
    assert eval_at(comp, z, trace_at, out["challenges"], hints) == provided
    assert eval_at(comp, z, trace_at, out["challenges"], [(hints[0] + 1) % P]) != provided
    # 2. the DEEP composition at the query positions is the first FRI layer there (src/verifier.rs:238-300)
    g, gen_l = Radix2EvaluationDomain(n).group_gen, Radix2EvaluationDomain(N, 7).group_gen
    layer0 = out["deep_lde"].columns[0].to_numpy()
    z_n = pow(z, ce, P)
    for i, pos in enumerate(positions):
        x = 7 * pow(gen_l, rev(pos, log_N), P) % P
        acc = 0
        for j, ((col, off), ood) in enumerate(zip(out["trace_args"], execution)):
            acc += deep.execution_trace[j] * (gl_from_mont(int(q.base_trace_values[i][col])) - ood) * pow((x - z * pow(g, off, P)) % P, -1, P)
        for j, ood in enumerate(composition):
            acc += deep.composition_trace[j] * (gl_from_mont(int(q.composition_trace_values[i][j])) - ood) * pow((x - z_n) % P, -1, P)
        assert gl_from_mont(int(layer0[pos])) == acc % P * ((deep.degree[0] + deep.degree[1] * x) % P) % P, f"query {i} at position {pos}"
    # 3. fri.rs:244: no remainder coefficient from n_rem / blowup on
    assert not high_remainder_coefficients(out, V=1).any() and out["remainder_coeffs"].any()
    # 4. FriVerifier::verify_generic + verify_remainder (src/fri.rs:346-490) on the layer openings
    gen, wf, size = Radix2EvaluationDomain(N).group_gen, Radix2EvaluationDomain(folding).group_gen, N
    evaluations = [gl_from_mont(int(layer0[p])) for p in positions]
    for opening, alpha in zip(out["fri_openings"], out["fri_alphas"]):
        folded = pipeline.fold_positions(positions, folding)
        rows = [canon(row) for row in opening["rows"]]
        assert [rows[folded.index(p // folding)][p % folding] for p in positions] == evaluations
        nxt = []
        for row, fp in zip(rows, folded):
            offset = pow(gen, rev(fp, (size // folding).bit_length() - 1), P)
            vals = [row[rev(k, log_f)] for k in range(folding)]
            coeffs = [sum(v * pow(offset * pow(wf, k, P) % P, -j, P) for k, v in enumerate(vals)) % P for j in range(folding)]
            nxt.append(sum(c * pow(alpha, j, P) for j, c in enumerate(coeffs)) % P)
        evaluations, positions, gen, size = nxt, folded, pow(gen, folding, P), size // folding
    rem = canon(out["remainder_coeffs"])
    assert len(rem) == max(size // BLOWUP, 1)
    for p, want in zip(positions, evaluations):
        x = pow(gen, rev(p, size.bit_length() - 1), P)
        assert sum(c * pow(x, j, P) for j, c in enumerate(rem)) % P == want


@pytest.mark.parametrize("kind", KINDS)
def test_an_fq3_proof_with_a_lookup_column(kind):
    out, comp, nair = lookup_proof(kind)
    assert all(isinstance(v, tuple) and len(v) == 3 for v in out["air_challenges"] + out["challenges"] + [out["z"]] + out["fri_alphas"])
    check_replay(out, nair, 3, 8)
    check_openings(out, 8)
    assert ood_consistent(out, comp)
    assert not high_remainder_coefficients(out).any() and out["remainder_coeffs"].any()


def _same(a, b):
    if hasattr(a, "to_numpy"):
        return type(a) is type(b) and _same(a.to_numpy(), b.to_numpy())
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, (int, str, bytes, type(None))):
        return a == b
    return type(a) is type(b) and _same({k: v for k, v in vars(a).items() if not k.startswith("_")}, {k: v for k, v in vars(b).items() if not k.startswith("_")})


@pytest.mark.parametrize("kind", KINDS)
def test_coin_none_is_the_prover_as_it_was(kind):
    pl, n = backends.planner(kind), 1 << LOG_T
    cols = fib_trace(n)
    trace = Matrix.from_numpy(pl, [np.array([gl_to_mont(v) for v in c], dtype=np.uint64) for c in cols], FP)
    comp, ce, nch = pipeline.fib_constraints(n, 8)
    args = (pl, trace, comp, nch, [cols[7][n - 1]], bytes(range(32)), BLOWUP, 8, MAXREM, BITS, NQ)
    without = pipeline.prove(*args, hash="rpo256", ce_blowup=ce)
    with_none = pipeline.prove(*args, hash="rpo256", ce_blowup=ce, coin=None)
    assert sorted(without) == sorted(with_none) and _same(without, with_none)
    assert not _same(without, dict(with_none, nonce=with_none["nonce"] + 1))                 # the comparison sees a difference
    algebraic = pipeline.prove(*args, hash="rpo256", ce_blowup=ce, coin="rpo256")           # 32 bytes: four little-endian words below p
    assert algebraic["base_root"] == without["base_root"] and algebraic["challenges"] != without["challenges"]
    assert pipeline.pow_hash("rpo256") == "sha256"


def test_the_algebraic_coin_needs_rpo_commitments_over_goldilocks():
    pl, n = backends.planner("emu"), 16
    cols = fib_trace(n)
    trace = Matrix.from_numpy(pl, [np.array([gl_to_mont(v) for v in c], dtype=np.uint64) for c in cols], FP)
    comp, ce, nch = pipeline.fib_constraints(n, 8)
    args = (pl, trace, comp, nch, [cols[7][n - 1]], SEED, BLOWUP, 8, MAXREM, BITS, NQ)
    with pytest.raises(ValueError, match='coin="rpo256"'):
        pipeline.prove(*args, hash="sha256", ce_blowup=ce, coin="rpo256")
    with pytest.raises(ValueError):
        pipeline.prove(*args, hash="rpo256", ce_blowup=ce, coin="rpo256", field=F252)
    with pytest.raises(ValueError, match="coin is None"):
        pipeline.prove(*args, hash="rpo256", ce_blowup=ce, coin="sha256")
    with pytest.raises(ValueError, match="below p"):
        pipeline.prove(pl, trace, comp, nch, [cols[7][n - 1]], b"\xff" * 32, BLOWUP, 8, MAXREM, BITS, NQ, hash="rpo256", ce_blowup=ce, coin="rpo256")
