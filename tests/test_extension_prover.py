"""`pipeline.prove` over the cubic extension, with an extension trace built between the two commitments: `permutation_air` (4 Fp + 3 Fq3
columns, 4 challenges drawn after the base commitment), and the fib AIR with fq = Fq3 and no extension trace.  Word for word:
  - the extension columns are the sequential loop (tests/ext_ref.py) on the challenges the proof reports;
  - the base, extension and composition roots are hashlib / oracle.pyref Merkle roots over the oracle's LDEs, the FRI roots over the layers;
  - tests/coin_ref.py replays the transcript from the proof's own roots, out-of-domain values, remainder and nonce, in the reference's
    order (base root, AIR challenges, extension root, composition coefficients, ...), and arrives at every draw;
  - the verifier's relations (tests/test_verifier_relations.py) hold over Fq3 with the extension columns included;
  - fri.rs:244: every remainder coefficient from index n_rem / blowup on is zero;
  - the same AIR with fq = Fp (interaction columns over the base field), and SHA3-256 next to SHA-256, BLAKE2s and RPO-256;
  - negative controls, one extension cell altered before the commitment: a cell of the committed extension LDE makes the remainder's high
    coefficients non-zero (what fri.rs:244 is there to catch: a commitment that is not of low degree); a cell of the extension TRACE makes
    the out-of-domain consistency check fail (what an invalid execution breaks)."""
import hashlib

import numpy as np
import pytest

from oracle import cref
from oracle.pyref import rpo
from oracle.pyref.fields import FQ3 as Q, GL
from tests import backends, coin_ref, keccak_ref
from tests.ext_ref import PAIRS, reference
from tests.test_verifier_relations import _q_eval_at, fib_trace
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, GpuVec, Matrix, Radix2EvaluationDomain, build_extension_columns, pipeline
from ministark_amd.api import GL_P as P, gl_from_mont, pow_hash

BLOWUP, FOLDING, MAXREM, BITS, NQ = 4, 4, 4, 8, 16
SEED = bytes(range(11, 43))
_proofs = {}


class AlteredLde(Matrix):
    """an extension trace whose LDE has one component of one cell of Q altered between the transform and the commitment"""

    def interpolate(self, domain):
        polys = Matrix.interpolate(self, domain)
        evaluate = polys.bit_reversed_evaluate

        def altered(lde_domain):
            lde = evaluate(lde_domain)
            w = lde.columns[1].to_numpy()
            at = 3 * (lde.num_rows() // 3) + 1
            w[at] = (int(w[at]) + 1) % P
            lde.columns[1] = GpuVec.from_numpy(lde.planner, w, FQ3F)
            return lde
        polys.bit_reversed_evaluate = altered
        return polys


def prove_permutation(kind, log_t, hash="sha256", tamper=False, fq=FQ3F):
    """tamper: False; "trace": one cell of the extension trace altered before it is interpolated and committed; "lde": one cell of the
    extension LDE altered before it is committed"""
    pl, n = backends.planner(kind), 1 << log_t
    cols = pipeline.permutation_trace(n, 40 + log_t)
    trace = Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols], FP)
    comp, ce, ncoef, nair, columns = pipeline.permutation_air(n)
    assert ce == 2 and nair == 4
    extension = columns
    if tamper == "lde":
        extension = lambda base, challenges: AlteredLde(build_extension_columns(pl, base, challenges, columns, FQ3F).columns)
    elif tamper:
        assert tamper == "trace"

        def extension(base, challenges):
            m = build_extension_columns(pl, base, challenges, columns, FQ3F)
            w = m.columns[1].to_numpy()
            w[3 * (n // 3) + 1] = (int(w[3 * (n // 3) + 1]) + 1) % P                    # one component of one cell of Q
            m.columns[1] = GpuVec.from_numpy(pl, w, FQ3F)
            return m
    out = pipeline.prove(pl, trace, comp, ncoef, [], SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash=hash, keep=True, ce_blowup=ce,
                         fq=fq, num_air_challenges=nair, extension=extension)
    return out, cols, comp, columns


def proof(kind, log_t, hash="sha256", fq=FQ3F):
    """one proof per case, shared by the tests and left unchanged"""
    key = (kind, log_t, hash, False, fq)
    if key not in _proofs:
        _proofs[key] = prove_permutation(*key)
    return _proofs[key]


def replay(out, hash, nair, seed=SEED, fq=FQ3F):
    """the verifier's side of the transcript over fq, from the proof's own contents -> every draw as canonical values (3-tuples over Fq3)"""
    vals = lambda words: pipeline.from_fq_words(fq, words)
    words = lambda values: pipeline.fq_words(fq, values).ravel()
    rf = coin_ref.FQ3 if fq == FQ3F else coin_ref.FP
    c = (keccak_ref.Coin if pow_hash(hash) in keccak_ref.DOMAIN else coin_ref.Coin)(seed, pow_hash(hash))
    got = {}
    c.reseed_digest(out["base_root"])
    got["air_challenges"] = vals(c.draw(rf, nair)) if nair else []
    if "extension_root" in out:
        c.reseed_digest(out["extension_root"])
    got["challenges"] = vals(c.draw(rf, len(out["challenges"])))
    c.reseed_digest(out["composition_root"])
    got["z"] = vals(c.draw(rf, 1))[0]
    c.reseed_elements(rf, words(list(out["ood"][0]) + list(out["ood"][1])))
    nexec, ncomp = len(out["ood"][0]), len(out["ood"][1])
    d = vals(c.draw(rf, nexec + ncomp + 2))
    got["deep"] = (d[:nexec], d[nexec: nexec + ncomp], (d[-2], d[-1]))
    got["fri_alphas"] = []
    for root in out["fri_roots"]:
        c.reseed_digest(root)
        got["fri_alphas"].append(vals(c.draw(rf, 1))[0])
    c.reseed_elements(rf, out["remainder_coeffs"])
    got["nonce"] = c.grind(BITS)
    c.reseed_int(out["nonce"])
    got["positions"] = c.draw_queries(NQ, len(out["remainder"]) * FOLDING ** len(out["fri_roots"]))
    return got


def check_replay(out, hash, nair, fq=FQ3F):
    got = replay(out, hash, nair, fq=fq)
    assert len(out["fri_roots"]) >= 1
    assert out["air_challenges"] == got["air_challenges"] and len(got["air_challenges"]) == nair
    assert out["challenges"] == got["challenges"]
    assert out["z"] == got["z"]
    assert (out["deep"].execution_trace, out["deep"].composition_trace, out["deep"].degree) == got["deep"]
    assert out["fri_alphas"] == got["fri_alphas"]
    assert out["nonce"] == got["nonce"]
    assert out["positions"] == got["positions"] and 1 <= len(got["positions"]) <= NQ


def high_remainder_coefficients(out, V=3):
    """the remainder polynomial's coefficients (V words each) from index n_rem / blowup on (fri.rs:244 asserts that they vanish)"""
    coeffs = out["remainder_poly"].to_numpy().reshape(-1, V)
    assert len(coeffs) == len(out["remainder"]) and len(coeffs) >= BLOWUP
    return coeffs[len(coeffs) // BLOWUP:]


# ---- roots: leaf = H(canonical little-endian bytes of the row), node = H(left || right); RPO-256 absorbs the row's Fp words ----------
def merkle_root(hash, rows):
    """rows: one list of canonical Fp integers per row (an Fq3 element is its three components)"""
    if hash == "rpo256":
        return np.array([GL.to_mont(v) for v in rpo.merkle_nodes([rpo.hash_row(r) for r in rows])[1]], dtype=np.uint64).tobytes()
    H = {"sha256": hashlib.sha256, "blake2s": hashlib.blake2s, "sha3_256": hashlib.sha3_256}[hash]
    level = [H(b"".join(int(v).to_bytes(8, "little") for v in r)).digest() for r in rows]
    while len(level) > 1:
        level = [H(level[2 * k] + level[2 * k + 1]).digest() for k in range(len(level) // 2)]
    return level[0]


def rows_of(columns_words, V):
    """bit-reversed LDE columns (Montgomery words, V per element) -> canonical rows"""
    canon = [cref.from_mont(c).reshape(-1, V) for c in columns_words]
    return [[int(v) for c in canon for v in c[r]] for r in range(len(canon[0]))]


def oracle_roots(out, cols, comp, log_t, hash):
    """base, extension and composition roots from the oracle's transforms and constraint evaluation, given the proof's challenges"""
    n, log_b, log_ce = 1 << log_t, BLOWUP.bit_length() - 1, 1
    base = [pipeline.to_mont_words(FP, c).ravel() for c in cols]
    ext = [PAIRS["fp_fq3"].ext_words(c) for c in reference(PAIRS["fp_fq3"], cols, out["air_challenges"], pipeline.permutation_air(n)[4])]
    roots = {"base_root": merkle_root(hash, rows_of([cref.lde(c, log_t, log_b, 1, 7, True) for c in base], 1)),
             "extension_root": merkle_root(hash, rows_of([cref.lde(c, log_t, log_b, 3, 7, True) for c in ext], 3))}
    ch = pipeline.fq_words(FQ3F, out["air_challenges"] + out["challenges"])
    base_ce = [cref.lde(c, log_t, log_ce, 1, 7, False) for c in base]
    ext_ce = [cref.lde(c, log_t, log_ce, 3, 7, False) for c in ext]
    evals = cref.eval_expr(comp, log_t + log_ce, 1 << log_ce, 7, base_ce, ext_ce, ch, ch[:1], True)
    poly = cref.ntt(evals, log_t + log_ce, 3, True, 7).reshape(-1, 3)
    N, log_N = n * BLOWUP, log_t + log_b
    comp_lde = []
    for c in range(1 << log_ce):
        a = np.zeros(3 * N, dtype=np.uint64)
        a[:3 * n] = np.ascontiguousarray(poly[c::1 << log_ce]).ravel()
        comp_lde.append(cref.bit_reverse(cref.ntt(a, log_N, 3, False, 7), log_N, 3))
    roots["composition_root"] = merkle_root(hash, rows_of(comp_lde, 3))
    return roots


def check_fri_roots(out, hash, V=3):
    for layer, root in zip(out["fri_layers"], out["fri_roots"]):
        assert merkle_root(hash, cref.from_mont(layer.to_numpy()).reshape(-1, V * FOLDING).tolist()) == root


# ---- the simulator: 2^6 rows -----------------------------------------------------------------------------------------------------------
LOG_T = 6


def test_extension_columns_are_the_sequential_loop_on_the_drawn_challenges():
    out, cols, _, columns = proof("emu", LOG_T)
    want = reference(PAIRS["fp_fq3"], cols, out["air_challenges"], columns)
    assert out["ext_trace"].num_cols() == 3
    for got, w in zip(out["ext_trace"].to_numpy(), want):
        assert np.array_equal(got, PAIRS["fp_fq3"].ext_words(w))
    # the AIR is valid on this trace: the two running products meet in the last row
    assert want[0][-1] == want[1][-1] and want[0][0] == want[1][0] == Q.one() and want[2][0] == Q.zero()


@pytest.mark.parametrize("hash", ["sha256", "blake2s", "rpo256", "sha3_256"])
def test_roots_are_the_oracle_roots_and_the_remainder_has_low_degree(hash):
    out, cols, comp, _ = proof("emu", LOG_T, hash)
    for name, root in oracle_roots(out, cols, comp, LOG_T, hash).items():
        assert out[name] == root, name
    check_fri_roots(out, hash)
    check_replay(out, hash, 4)
    assert not high_remainder_coefficients(out).any()


def ood_consistent(out, comp):
    """the verifier's out-of-domain consistency check (src/verifier.rs:82-95) over Fq3: the constraints evaluated at z from the reported
    trace values against the reported composition-trace values"""
    execution = [tuple(int(w) for w in v) for v in out["ood"][0]]
    calculated = _q_eval_at(comp, out["z"], dict(zip(out["trace_args"], execution)), out["air_challenges"] + out["challenges"])
    provided, zk = Q.zero(), Q.one()
    for h in out["ood"][1]:
        provided, zk = Q.add(provided, Q.mul(tuple(int(w) for w in h), zk)), Q.mul(zk, out["z"])
    return calculated == provided


def test_an_altered_extension_cell_breaks_the_low_degree_of_the_remainder():
    """The negative control of the remainder check: with one cell of the committed extension matrix -- its LDE -- altered before the
    commitment, the column is no longer of degree < n, the DEEP evaluations computed from the committed rows are not either, the change
    travels through every fold into one value of the remainder, and the remainder's high coefficients are not all zero.  (A cell of the
    extension TRACE cannot do this: the altered column is still interpolated, so its LDE has degree < n; the composition trace is
    interpolated from its evaluations, so it has too; and every DEEP quotient (T(x) - T(z)) / (x - z) of a polynomial is a polynomial.  All
    36 high remainder words stay zero then -- asserted below -- and what breaks is the out-of-domain consistency, the next test.)"""
    out, _, _, _ = prove_permutation("emu", LOG_T, tamper="lde")
    check_replay(out, "sha256", 4)                                     # the transcript is still the transcript of what was committed
    assert out["extension_root"] != proof("emu", LOG_T)[0]["extension_root"] and out["base_root"] == proof("emu", LOG_T)[0]["base_root"]
    assert high_remainder_coefficients(out).any()
    assert not high_remainder_coefficients(prove_permutation("emu", LOG_T, tamper="trace")[0]).any()


def test_an_altered_extension_trace_cell_breaks_the_out_of_domain_consistency():
    out, _, comp, _ = prove_permutation("emu", LOG_T, tamper="trace")
    check_replay(out, "sha256", 4)
    assert out["extension_root"] != proof("emu", LOG_T)[0]["extension_root"] and out["base_root"] == proof("emu", LOG_T)[0]["base_root"]
    assert not ood_consistent(out, comp)
    assert ood_consistent(proof("emu", LOG_T)[0], comp)


def test_verifier_relations_hold_over_fq3_with_the_extension_columns():
    out, _, comp, _ = proof("emu", LOG_T)
    n, N = 1 << LOG_T, (1 << LOG_T) * BLOWUP
    args, z, coeffs = out["trace_args"], out["z"], out["deep"]
    assert args == [(c, o) for c in range(7) for o in (0, 1)]
    execution = [tuple(int(w) for w in v) for v in out["ood"][0]]
    composition = [tuple(int(w) for w in v) for v in out["ood"][1]]
    # 1. out-of-domain consistency (src/verifier.rs:82-95)
    assert ood_consistent(out, comp)
    # 2. the DEEP composition at the queried rows (src/verifier.rs:238-300)
    trace_dom, lde_dom = Radix2EvaluationDomain(n), Radix2EvaluationDomain(N, 7)
    g, z_n, log_N = trace_dom.group_gen, Q.pow(z, len(composition)), N.bit_length() - 1
    from_words = lambda row, k: tuple(gl_from_mont(int(w)) for w in row[3 * k: 3 * k + 3])
    deep_lde = out["deep_lde"].columns[0].to_numpy().reshape(-1, 3)
    q = out["queries"]
    for i, pos in enumerate(out["positions"]):
        xv = 7 * pow(lde_dom.group_gen, int(format(pos, f"0{log_N}b")[::-1], 2), P) % P
        acc = Q.zero()
        for j, ((col, off), ood) in enumerate(zip(args, execution)):
            value = Q.embed(gl_from_mont(int(q.base_trace_values[i][col]))) if col < 4 else from_words(q.extension_trace_values[i], col - 4)
            acc = Q.add(acc, Q.mul(Q.mul(coeffs.execution_trace[j], Q.sub(value, ood)), Q.inv(Q.sub(Q.embed(xv), Q.mul_base(z, pow(g, off, P))))))
        for j, ood in enumerate(composition):
            acc = Q.add(acc, Q.mul(Q.mul(coeffs.composition_trace[j], Q.sub(from_words(q.composition_trace_values[i], j), ood)), Q.inv(Q.sub(Q.embed(xv), z_n))))
        assert tuple(gl_from_mont(int(w)) for w in deep_lde[pos]) == Q.mul(acc, Q.add(coeffs.degree[0], Q.mul_base(coeffs.degree[1], xv))), (i, pos)


@pytest.mark.parametrize("kind,log_t", [pytest.param("emu", LOG_T, id="emu"), pytest.param("hip", 10, id="hip", marks=pytest.mark.gpu)])
def test_permutation_air_as_an_fq_equal_fp_air_with_interaction_columns(kind, log_t):
    """fq = the base field with an extension trace: the evaluator takes base and interaction columns as ONE table of Fp columns, the
    challenges are Fp elements, everything after is the Fq = Fp prover's.  Same checks as over Fq3."""
    out, cols, _, columns = proof(kind, log_t, fq=FP)
    pair, log_b = PAIRS["fp_fp"], BLOWUP.bit_length() - 1
    assert all(isinstance(v, int) for v in out["air_challenges"] + [out["z"]]) and out["trace_args"] == [(c, o) for c in range(7) for o in (0, 1)]
    want = reference(pair, cols, out["air_challenges"], columns)
    assert want[0][-1] == want[1][-1]
    assert out["ext_trace"].field == FP and all(np.array_equal(g, pair.ext_words(w)) for g, w in zip(out["ext_trace"].to_numpy(), want))
    lde_root = lambda columns_: merkle_root("sha256", rows_of([cref.lde(pair.base_words(c), log_t, log_b, 1, 7, True) for c in columns_], 1))
    assert out["base_root"] == lde_root(cols) and out["extension_root"] == lde_root(want)
    check_fri_roots(out, "sha256", V=1)
    check_replay(out, "sha256", 4, fq=FP)
    assert not high_remainder_coefficients(out, V=1).any() and out["remainder_coeffs"].any()
    assert out["base_root"] == proof(kind, log_t)[0]["base_root"] and out["extension_root"] != proof(kind, log_t)[0]["extension_root"]


def prove_fib_fq3(kind, log_t):
    pl, n = backends.planner(kind), 1 << log_t
    cols = fib_trace(n)
    trace = Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols], FP)
    comp, ce, nch = pipeline.fib_constraints(n)
    return pipeline.prove(pl, trace, comp, nch, [cols[7][n - 1]], SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, keep=True, ce_blowup=ce, fq=FQ3F)


def test_fib_over_fq3_without_an_extension_trace():
    out = prove_fib_fq3("emu", LOG_T)
    assert "extension_root" not in out and "ext_trace" not in out and isinstance(out["z"], tuple)
    check_replay(out, "sha256", 0)
    check_fri_roots(out, "sha256")
    assert not high_remainder_coefficients(out).any()
    # the base commitment does not depend on fq: it is the Fq = Fp prover's
    pl = backends.planner("emu")
    cols = fib_trace(1 << LOG_T)
    trace = Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols], FP)
    comp, ce, nch = pipeline.fib_constraints(1 << LOG_T)
    plain = pipeline.prove(pl, trace, comp, nch, [cols[7][-1]], SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, ce_blowup=ce)
    assert plain["base_root"] == out["base_root"] and isinstance(plain["z"], int) and plain["air_challenges"] == []


# ---- the device: 2^10 rows, and 2^15 rows whose 2^16-point evaluation domain takes the specialised evaluator ---------------------------
def same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


@pytest.mark.gpu
@pytest.mark.parametrize("log_t", [10, 15])
def test_permutation_air_on_the_device(log_t):
    out, cols, comp, columns = proof("hip", log_t)
    check_replay(out, "sha256", 4)
    assert not high_remainder_coefficients(out).any()
    if log_t == 10:
        want = reference(PAIRS["fp_fq3"], cols, out["air_challenges"], columns)
        assert all(np.array_equal(got, PAIRS["fp_fq3"].ext_words(w)) for got, w in zip(out["ext_trace"].to_numpy(), want))
        for name, root in oracle_roots(out, cols, comp, log_t, "sha256").items():
            assert out[name] == root, name
    again, _, _, _ = prove_permutation("hip", log_t)
    for key in ("base_root", "extension_root", "composition_root", "fri_roots", "ood", "remainder_coeffs", "nonce", "positions", "z", "challenges",
                "air_challenges", "fri_alphas"):
        assert same(out[key], again[key]), key
    assert np.array_equal(out["remainder"].to_numpy(), again["remainder"].to_numpy())
    for member in ("base_trace_values", "extension_trace_values", "composition_trace_values"):
        assert np.array_equal(getattr(out["queries"], member), getattr(again["queries"], member)), member


@pytest.mark.gpu
def test_fib_over_fq3_on_the_device():
    out = prove_fib_fq3("hip", 10)
    check_replay(out, "sha256", 0)
    assert not high_remainder_coefficients(out).any()
