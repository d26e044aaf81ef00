"""`pipeline.range_trace_on_device` and `pipeline.range_air`: a range-checked trace whose limb columns are written by ms_limb_decompose and
whose m column is counted by ms_range_multiplicities, both where the trace lies -- in the manner of tests/test_lookup_prover.py, whose
helpers it uses:
  - the device-built trace is the uploaded `range_trace` in every word;
  - debug.validate_constraints accepts it under `range_air`;
  - `pipeline.prove` on it gives every reported value of the proof on the host-built trace.  The cleared LogUp transition has degree 4:
    `range_air` returns ce_blowup = 4, and the proofs here run at blowup = 4 (tests/test_extension_prover.py's BLOWUP);
  - negative control: one x at or above 2^(2 bits).  `check=True` raises LookupMissing naming that row and that value; without the check,
    validate_constraints fails at the recomposition constraint, at that row."""
import numpy as np
import pytest

from tests import backends
from tests.logup_ref import PAIRS
from tests.test_extension_prover import BITS, BLOWUP, FOLDING, MAXREM, NQ, SEED
from tests.test_lookup_prover import REPORTED, same
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, GpuVec, LookupMissing, Matrix, build_extension_columns, debug, pipeline

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
SIZES = [pytest.param("emu", 10, id="emu"), pytest.param("hip", 12, id="hip", marks=pytest.mark.gpu)]
LIMB_BITS = 8
RECOMPOSITION, BOUNDARY, TRANSITION = 0, 1, 2
CHAL = [(3, 1, 4)]


def upload(pl, cols):
    return Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols], FP)


def test_the_host_built_trace_is_what_its_docstring_says():
    n, bits = 64, 5
    x, l0, l1, t, m = pipeline.range_trace(n, bits, 5)
    assert all(0 <= v < 1 << (2 * bits) and v == a + (b << bits) and a < 1 << bits and b < 1 << bits for v, a, b in zip(x, l0, l1))
    assert t == list(range(32)) + [31] * 32 and m == [(l0 + l1).count(j) for j in range(32)] + [0] * 32 and sum(m) == 2 * n and max(l1) > 0
    with pytest.raises(AssertionError):
        pipeline.range_trace(16, 5, 5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,bits", [(16, 2), (256, 8), (1024, 8), (1024, 10)])
def test_the_device_built_trace_is_the_host_built_trace_and_satisfies_the_air(kind, n, bits):
    pl = backends.planner(kind)
    want = [pipeline.to_mont_words(FP, c).ravel() for c in pipeline.range_trace(n, bits, 30 + n)]
    assert any(want[1]) and any(want[2]) and any(want[4])
    got = pipeline.range_trace_on_device(pl, n, bits, 30 + n, check=True)
    assert got.num_cols() == 5 and got.field == FP
    for c, (g, w) in enumerate(zip(got.to_numpy(), want)):
        assert np.array_equal(g, w), c
    comp, ce, ncoef, nair, columns = pipeline.range_air(n, bits)
    assert (ce, nair, len(columns), ncoef) == (4, 1, 1, 6) and ce <= BLOWUP
    built = build_extension_columns(pl, got, GpuVec.from_numpy(pl, PAIRS["fp_fq3"].ext_words(CHAL), FQ3F), columns, FQ3F)
    assert debug.validate_constraints(pipeline.range_air_constraints(n, bits), CHAL, [], got, built).ok


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_the_proof_on_it_is_the_proof_on_the_host_built_trace(kind, log_t):
    pl, n = backends.planner(kind), 1 << log_t
    comp, ce, ncoef, nair, columns = pipeline.range_air(n, LIMB_BITS)
    prove = lambda trace: pipeline.prove(pl, trace, comp, ncoef, [], SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash="sha256", keep=True, ce_blowup=ce,
                                         fq=FQ3F, num_air_challenges=nair, extension=columns)
    host = prove(upload(pl, pipeline.range_trace(n, LIMB_BITS, 30 + log_t)))
    trace = pipeline.range_trace_on_device(pl, n, LIMB_BITS, 30 + log_t)
    out = prove(trace)
    for key in REPORTED:
        assert same(out[key], host[key]), key
    assert np.array_equal(out["ext_trace"].to_numpy()[0], host["ext_trace"].to_numpy()[0])
    assert debug.validate_constraints(pipeline.range_air_constraints(n, LIMB_BITS), out["air_challenges"], [], trace, out["ext_trace"]).ok


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_a_value_that_does_not_fit_its_limbs_is_named(kind, log_t):
    pl, n, bits = backends.planner(kind), 1 << log_t, LIMB_BITS
    x = list(pipeline.range_trace(n, bits, 30 + log_t)[0])
    row, stray = n // 3, (1 << (2 * bits)) + 0x1234
    x[row] = stray
    with pytest.raises(LookupMissing) as err:
        pipeline.range_trace_on_device(pl, n, bits, 30 + log_t, check=True, x=x)
    assert (err.value.spec, err.value.row, err.value.value, err.value.missing) == (0, row, stray, 1)
    assert f"row {row}" in str(err.value) and str(stray) in str(err.value)
    # without the check the call goes through: the row gets its low limbs, both in range, so the lookup is satisfied and only the
    # recomposition constraint sees the value -- at that row
    trace = pipeline.range_trace_on_device(pl, n, bits, 30 + log_t, x=x)
    limbs = [c.to_numpy()[row] for c in trace.columns[1:3]]
    assert limbs == [int(pipeline.to_mont_words(FP, [v]).ravel()[0]) for v in (0x34, 0x12)]
    comp, ce, ncoef, nair, columns = pipeline.range_air(n, bits)
    built = build_extension_columns(pl, trace, GpuVec.from_numpy(pl, PAIRS["fp_fq3"].ext_words(CHAL), FQ3F), columns, FQ3F)
    failed = debug.validate_constraints(pipeline.range_air_constraints(n, bits), CHAL, [], trace, built, raise_on_failure=False)
    assert failed.failures == [(RECOMPOSITION, row, 1)]
    with pytest.raises(debug.ConstraintViolation) as bad:
        debug.validate_constraints(pipeline.range_air_constraints(n, bits), CHAL, [], trace, built)
    assert (bad.value.constraint, bad.value.row) == (RECOMPOSITION, row)


@pytest.mark.parametrize("kind", KINDS)
def test_a_limb_column_that_was_tampered_with_is_named_by_the_count(kind):
    """a limb at or above 2^bits, written by hand into the trace: ms_range_multiplicities reports it missing, by set, row and value"""
    from ministark_amd import RangeSet, range_multiplicities
    pl, n, bits = backends.planner(kind), 256, 6
    cols = pipeline.range_trace(n, bits, 9)
    cols[2][77] = 64
    trace = upload(pl, cols[:4] + [[0] * n])
    _, report = range_multiplicities(pl, trace, bits, [RangeSet(1), RangeSet(2)], out=trace.columns[4])
    with pytest.raises(LookupMissing) as err:
        report.check()
    assert (err.value.set, err.value.row, err.value.values, err.value.missing) == (1, 77, [64], 1)
