"""`pipeline.prove` with a logarithmic-derivative lookup: `lookup_air` (5 Fp columns a0, a1, t0, t1, m + 1 Fq3 running sum S, challenges
alpha, beta drawn after the base commitment), S built by ms_build_logup_columns between the two commitments.  In the manner of
tests/test_extension_prover.py, whose helpers it uses, word for word:
  - the extension column is the sequential loop (tests/logup_ref.py) on the challenges the proof reports;
  - the base, extension and composition roots are the oracle's, over SHA-256 and BLAKE2s; tests/coin_ref.py replays every draw;
  - every remainder coefficient from index n_rem / blowup on is zero; the out-of-domain consistency relation holds;
  - debug.validate_constraints passes on (base, built extension);
  - negative controls: (i) a looked-up pair that is not in the table -- the transition fails at the LAST row, where Trace(S, 1) wraps to
    row 0 and the total is not zero, and the proof's out-of-domain consistency fails; (ii) alpha = t0[5] + beta t1[5] handed in directly --
    the builder writes the inv(0) = 0 increment and the transition fails at row 5 first (and on the rows that look table row 5 up);
  - permutation_air's ExtColumns and a LogUpColumn in ONE build_extension_columns call come back in the order listed;
  - the same AIR with fq = Fp."""
import numpy as np
import pytest

from oracle import cref
from oracle.pyref.fields import FQ3 as Q
from tests import backends, ext_ref, logup_ref
from tests.logup_ref import PAIRS
from tests.test_extension_prover import (BITS, BLOWUP, FOLDING, MAXREM, NQ, SEED, check_fri_roots, check_replay, high_remainder_coefficients,
                                         merkle_root, ood_consistent, rows_of)
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, GpuVec, Matrix, build_extension_columns, debug, pipeline
from ministark_amd.api import GL_P as P

LOG_T = 6                                  # the simulator's size (tests/test_extension_prover.py's); the device runs 2^10 rows
SIZES = [pytest.param("emu", LOG_T, id="emu"), pytest.param("hip", 10, id="hip", marks=pytest.mark.gpu)]
TRANSITION = 1                             # the index of the transition constraint in lookup_air_constraints
_proofs = {}


def lookup_columns(n, log_t, stray=False):
    """the base trace; stray: row 3 looks up a pair that is not a row of the table"""
    cols = pipeline.lookup_trace(n, 70 + log_t)
    if stray:
        cols[0] = list(cols[0])
        cols[0][3] = (cols[0][3] + 1) % P
        assert (cols[0][3], cols[1][3]) not in set(zip(cols[2], cols[3]))
    return cols


def prove_lookup(kind, log_t, hash="sha256", fq=FQ3F, stray=False):
    pl, n = backends.planner(kind), 1 << log_t
    cols = lookup_columns(n, log_t, stray)
    trace = Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols], FP)
    comp, ce, ncoef, nair, columns = pipeline.lookup_air(n)
    assert nair == 2 and len(columns) == 1 and ce <= BLOWUP
    out = pipeline.prove(pl, trace, comp, ncoef, [], SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash=hash, keep=True, ce_blowup=ce,
                         fq=fq, num_air_challenges=nair, extension=columns)
    return out, cols, comp, columns, ce, trace


def proof(kind, log_t, hash="sha256", fq=FQ3F):
    """one proof per case, shared by the tests and left unchanged"""
    key = (kind, log_t, hash, fq)
    if key not in _proofs:
        _proofs[key] = prove_lookup(*key)
    return _proofs[key]


def oracle_roots(out, cols, comp, columns, ce, log_t, hash):
    """base, extension and composition roots from the oracle's transforms and constraint evaluation, given the proof's challenges"""
    n, log_b, log_ce = 1 << log_t, BLOWUP.bit_length() - 1, ce.bit_length() - 1
    base = [pipeline.to_mont_words(FP, c).ravel() for c in cols]
    ext = [PAIRS["fp_fq3"].ext_words(c) for c in logup_ref.reference(PAIRS["fp_fq3"], cols, out["air_challenges"], columns)]
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


def test_the_lookup_trace_has_unused_and_repeated_table_rows():
    n = 1 << LOG_T
    a0, a1, t0, t1, m = pipeline.lookup_trace(n, 70 + LOG_T)
    table = list(zip(t0, t1))
    assert len(set(table)) == n and all(pair in table for pair in zip(a0, a1))
    assert m == [list(zip(a0, a1)).count(row) for row in table] and sum(m) == n
    assert 0 in m and max(m) >= 2 and m[5] >= 1                               # m[5]: what negative control (ii) leans on
    comp, ce, ncoef, nair, columns = pipeline.lookup_air(n)
    assert (ce, ncoef, nair) == (2, 4, 2) and ce == pipeline.composition_constraint(n, pipeline.lookup_air_constraints(n), 2)[1]


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_the_lookup_column_is_the_sequential_loop_on_the_drawn_challenges(kind, log_t):
    out, cols, _, columns, _, trace = proof(kind, log_t)
    want = logup_ref.reference(PAIRS["fp_fq3"], cols, out["air_challenges"], columns)
    assert out["ext_trace"].num_cols() == 1 and out["ext_trace"].field == FQ3F
    assert np.array_equal(out["ext_trace"].to_numpy()[0], PAIRS["fp_fq3"].ext_words(want[0]))
    # the AIR is valid on this trace: S starts at zero and the last row's increment brings it back to zero
    alpha, beta = out["air_challenges"]
    d = lambda x0, x1: Q.sub(Q.sub(alpha, Q.embed(x0)), Q.mul_base(beta, x1))
    last = Q.sub(Q.mul_base(logup_ref.inverse(PAIRS["fp_fq3"], d(cols[2][-1], cols[3][-1])), cols[4][-1]), logup_ref.inverse(PAIRS["fp_fq3"], d(cols[0][-1], cols[1][-1])))
    assert want[0][0] == Q.zero() and Q.add(want[0][-1], last) == Q.zero() and want[0][1] != Q.zero()
    report = debug.validate_constraints(pipeline.lookup_air_constraints(1 << log_t), out["air_challenges"], [], trace, out["ext_trace"])
    assert report.ok and report.unused_columns == [] and report.unused_challenges == []


@pytest.mark.parametrize("kind,log_t", SIZES)
@pytest.mark.parametrize("hash", ["sha256", "blake2s"])
def test_roots_are_the_oracle_roots_and_the_remainder_has_low_degree(kind, log_t, hash):
    out, cols, comp, columns, ce, _ = proof(kind, log_t, hash)
    for name, root in oracle_roots(out, cols, comp, columns, ce, log_t, hash).items():
        assert out[name] == root, name
    check_fri_roots(out, hash)
    check_replay(out, hash, 2)
    assert not high_remainder_coefficients(out).any() and out["remainder_coeffs"].any()
    assert ood_consistent(out, comp)


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_a_pair_that_is_not_in_the_table_fails_at_the_wrap_and_breaks_the_out_of_domain_consistency(kind, log_t):
    n = 1 << log_t
    out, cols, comp, columns, _, trace = prove_lookup(kind, log_t, stray=True)
    check_replay(out, "sha256", 2)                                             # the transcript is still the transcript of what was committed
    assert out["base_root"] != proof(kind, log_t)[0]["base_root"]
    want = logup_ref.reference(PAIRS["fp_fq3"], cols, out["air_challenges"], columns)
    assert np.array_equal(out["ext_trace"].to_numpy()[0], PAIRS["fp_fq3"].ext_words(want[0]))       # the builder did what the rule says
    report = debug.validate_constraints(pipeline.lookup_air_constraints(n), out["air_challenges"], [], trace, out["ext_trace"], raise_on_failure=False)
    assert report.failures == [(TRANSITION, n - 1, 1)]                          # every row's step holds; the total is not zero
    with pytest.raises(debug.ConstraintViolation) as err:
        debug.validate_constraints(pipeline.lookup_air_constraints(n), out["air_challenges"], [], trace, out["ext_trace"])
    assert (err.value.constraint, err.value.row) == (TRANSITION, n - 1)
    assert not ood_consistent(out, comp)
    assert ood_consistent(proof(kind, log_t)[0], comp)


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_a_zero_denominator_gets_the_zero_increment_and_fails_at_its_row(kind, log_t):
    """alpha = t0[5] + beta t1[5]: Dt vanishes on row 5 (and on no other row: the table's pairs are distinct)"""
    pl, n, pair = backends.planner(kind), 1 << log_t, PAIRS["fp_fq3"]
    cols = lookup_columns(n, log_t)
    assert cols[4][5] >= 1
    beta = (0x1234567, 89, 1011)
    alpha = Q.add(Q.embed(cols[2][5]), Q.mul_base(beta, cols[3][5]))
    trace = Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols], FP)
    columns = pipeline.lookup_air(n)[4]
    built = build_extension_columns(pl, trace, GpuVec.from_numpy(pl, pair.ext_words([alpha, beta]), FQ3F), columns, FQ3F)
    want = logup_ref.reference(pair, cols, [alpha, beta], columns)
    assert np.array_equal(built.to_numpy()[0], pair.ext_words(want[0]))
    da5 = Q.sub(Q.sub(alpha, Q.embed(cols[0][5])), Q.mul_base(beta, cols[1][5]))
    assert Q.sub(want[0][6], want[0][5]) == Q.neg(logup_ref.inverse(pair, da5))              # m / 0 contributed nothing
    report = debug.validate_constraints(pipeline.lookup_air_constraints(n), [alpha, beta], [], trace, built, raise_on_failure=False)
    # Da vanishes too, on the m[5] rows that look table row 5 up (all of them behind row 5 in this trace): there the builder drops 1 / Da and
    # the transition is left with Dt != 0.  With every term of table row 5 gone from both sides the total is still zero: the wrap holds.
    lookers = [i for i in range(n) if (cols[0][i], cols[1][i]) == (cols[2][5], cols[3][5])]
    assert len(lookers) == cols[4][5] and min(lookers) > 5 and n - 1 not in lookers
    assert report.failures == [(TRANSITION, 5, 1 + len(lookers))]


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_affine_and_logup_columns_mix_in_one_call_and_keep_their_order(kind, log_t):
    pl, n, pair = backends.planner(kind), 1 << log_t, PAIRS["fp_fq3"]
    cols = lookup_columns(n, log_t)
    trace = Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols], FP)
    affine, lookup = pipeline.permutation_air(n)[4], pipeline.lookup_air(n)[4]
    chal = pair.random_ext(np.random.default_rng(5), 4)
    d_chal = GpuVec.from_numpy(pl, pair.ext_words(chal), FQ3F)
    mixed = [affine[0], lookup[0], affine[1], affine[2]]
    got = build_extension_columns(pl, trace, d_chal, mixed, FQ3F)
    assert got.num_cols() == 4
    want_affine = ext_ref.reference(pair, cols, chal, affine)
    want_lookup = logup_ref.reference(pair, cols, chal, lookup)
    for g, w in zip(got.to_numpy(), [want_affine[0], want_lookup[0], want_affine[1], want_affine[2]]):
        assert np.array_equal(g, pair.ext_words(w))
    # each kind alone gives the same columns; into caller-provided outputs too
    outs = [GpuVec(pl, n, FQ3F) for _ in mixed]
    assert build_extension_columns(pl, trace, d_chal, mixed, FQ3F, out=outs).columns == outs
    assert all(np.array_equal(a, b) for a, b in zip(Matrix(outs).to_numpy(), got.to_numpy()))
    alone = build_extension_columns(pl, trace, d_chal, affine, FQ3F).to_numpy()
    assert all(np.array_equal(g, pair.ext_words(w)) for g, w in zip(alone, want_affine))


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_lookup_air_as_an_fq_equal_fp_air(kind, log_t):
    """fq = the base field: S is an Fp interaction column, the challenges are Fp elements.  Same checks as over Fq3."""
    out, cols, _, columns, _, _ = proof(kind, log_t, fq=FP)
    pair, log_b = PAIRS["fp_fp"], BLOWUP.bit_length() - 1
    assert all(isinstance(v, int) for v in out["air_challenges"] + [out["z"]])
    want = logup_ref.reference(pair, cols, out["air_challenges"], columns)
    assert want[0][0] == 0 and want[0][1] != 0
    assert out["ext_trace"].field == FP and np.array_equal(out["ext_trace"].to_numpy()[0], pair.ext_words(want[0]))
    lde_root = lambda columns_: merkle_root("sha256", rows_of([cref.lde(pair.base_words(c), log_t, log_b, 1, 7, True) for c in columns_], 1))
    assert out["base_root"] == lde_root(cols) and out["extension_root"] == lde_root(want)
    check_fri_roots(out, "sha256", V=1)
    check_replay(out, "sha256", 2, fq=FP)
    assert not high_remainder_coefficients(out, V=1).any() and out["remainder_coeffs"].any()
    assert out["base_root"] == proof(kind, log_t)[0]["base_root"] and out["extension_root"] != proof(kind, log_t)[0]["extension_root"]
