"""`pipeline.bitwise_trace_on_device` and `pipeline.bitwise_air`: a trace whose result column is written by ms_bitwise_columns, whose limb
columns by ms_limb_decompose, whose table by ms_bitwise_table and whose m column is counted by ms_bitwise_multiplicities, all where the trace
lies -- in the manner of tests/test_range_prover.py, for each of the three ops at n = 512 rows and 4-bit limbs:
  - the device-built trace is the uploaded `bitwise_trace` in every word;
  - debug.validate_constraints accepts it under `bitwise_air`;
  - `pipeline.prove` on it gives every reported value of the proof on the host-built trace.  The cleared LogUp transition has degree 4:
    `bitwise_air` returns ce_blowup = 4, and the proofs here run at blowup = 4 (tests/test_extension_prover.py's BLOWUP);
  - negative control: one bit of c flipped in one row.  `check=True` raises LookupMissing naming that row and its three values; without
    the check, validate_constraints names the LogUp transition, which no longer closes."""
import numpy as np
import pytest

from tests import backends
from tests.logup_ref import PAIRS
from tests.test_extension_prover import BITS, BLOWUP, FOLDING, MAXREM, NQ, SEED
from tests.test_lookup_prover import REPORTED, same
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, GpuVec, LookupMissing, Matrix, build_extension_columns, debug, pipeline

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
OPS = ["and", "or", "xor"]
N, LIMB_BITS = 512, 4
RECOMPOSITION_C, BOUNDARY, TRANSITION = 2, 3, 4
CHAL = [(3, 1, 4), (5, 9, 2), (6, 5, 3)]


def upload(pl, cols):
    return Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols], FP)


def test_the_host_built_trace_is_what_its_docstring_says():
    n, bits = 64, 3
    for op, fn in (("and", lambda x, y: x & y), ("or", lambda x, y: x | y), ("xor", lambda x, y: x ^ y)):
        a, b, c, a0, a1, b0, b1, c0, c1, tx, ty, tz, m = pipeline.bitwise_trace(n, bits, op, 5)
        assert all(x < 64 and y < 64 and z == fn(x, y) for x, y, z in zip(a, b, c))
        assert all(v == l0 + (l1 << bits) and l0 < 8 and l1 < 8 for v, l0, l1 in ((v, l0, l1) for col, lo, hi in ((a, a0, a1), (b, b0, b1), (c, c0, c1)) for v, l0, l1 in zip(col, lo, hi)))
        assert tx == [j >> 3 for j in range(64)] and ty == [j & 7 for j in range(64)] and tz == [fn(x, y) for x, y in zip(tx, ty)]
        pairs = [(x << bits) + y for x, y in zip(a0 + a1, b0 + b1)]
        assert m == [pairs.count(j) for j in range(64)] and sum(m) == 2 * n
    assert len(pipeline.BITWISE_COLUMNS) == 13
    t = pipeline.bitwise_trace(80, 3, "xor", 5)
    assert t[9][63:] == [7] * 17 and t[10][63:] == [7] * 17 and t[11][63:] == [0] * 17 and t[12][64:] == [0] * 16      # the last table row repeated
    with pytest.raises(AssertionError):
        pipeline.bitwise_trace(63, 3, "xor", 5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", OPS)
def test_the_device_built_trace_is_the_host_built_trace_and_satisfies_the_air(kind, op):
    pl = backends.planner(kind)
    want = [pipeline.to_mont_words(FP, c).ravel() for c in pipeline.bitwise_trace(N, LIMB_BITS, op, 30)]
    assert all(any(w) for w in want)
    got = pipeline.bitwise_trace_on_device(pl, N, LIMB_BITS, op, 30, check=True)
    assert got.num_cols() == 13 and got.field == FP
    for c, (g, w) in enumerate(zip(got.to_numpy(), want)):
        assert np.array_equal(g, w), pipeline.BITWISE_COLUMNS[c]
    comp, ce, ncoef, nair, columns = pipeline.bitwise_air(N, LIMB_BITS, op)
    assert (ce, nair, len(columns), ncoef) == (4, 3, 1, 10) and ce <= BLOWUP
    built = build_extension_columns(pl, got, GpuVec.from_numpy(pl, PAIRS["fp_fq3"].ext_words(CHAL), FQ3F), columns, FQ3F)
    assert debug.validate_constraints(pipeline.bitwise_air_constraints(N, LIMB_BITS), CHAL, [], got, built).ok


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", OPS)
def test_the_proof_on_it_is_the_proof_on_the_host_built_trace(kind, op):
    pl = backends.planner(kind)
    comp, ce, ncoef, nair, columns = pipeline.bitwise_air(N, LIMB_BITS, op)
    prove = lambda trace: pipeline.prove(pl, trace, comp, ncoef, [], SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash="sha256", keep=True, ce_blowup=ce,
                                         fq=FQ3F, num_air_challenges=nair, extension=columns)
    host = prove(upload(pl, pipeline.bitwise_trace(N, LIMB_BITS, op, 31)))
    trace = pipeline.bitwise_trace_on_device(pl, N, LIMB_BITS, op, 31)
    out = prove(trace)
    for key in REPORTED:
        assert same(out[key], host[key]), key
    assert np.array_equal(out["ext_trace"].to_numpy()[0], host["ext_trace"].to_numpy()[0])
    assert debug.validate_constraints(pipeline.bitwise_air_constraints(N, LIMB_BITS), out["air_challenges"], [], trace, out["ext_trace"]).ok


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", OPS)
def test_one_flipped_bit_of_c_is_named(kind, op):
    pl = backends.planner(kind)
    a, b, c = (list(col) for col in pipeline.bitwise_trace(N, LIMB_BITS, op, 32)[:3])
    row = N // 3
    c[row] ^= 1 << 5
    with pytest.raises(LookupMissing) as err:
        pipeline.bitwise_trace_on_device(pl, N, LIMB_BITS, op, 32, check=True, c=c)
    assert (err.value.set, err.value.row, err.value.values, err.value.missing) == (0, row, [a[row], b[row], c[row]], 1)
    assert f"row {row}" in str(err.value) and f"c = {c[row]}" in str(err.value) and op in str(err.value)
    # without the check the call goes through: the row's limbs recompose to the wrong c, none of its limb pairs is counted into m, and its
    # high limb triple is no table row -- the fractions no longer sum to zero, which the transition sees where the sum wraps around
    trace = pipeline.bitwise_trace_on_device(pl, N, LIMB_BITS, op, 32, c=c)
    comp, ce, ncoef, nair, columns = pipeline.bitwise_air(N, LIMB_BITS, op)
    built = build_extension_columns(pl, trace, GpuVec.from_numpy(pl, PAIRS["fp_fq3"].ext_words(CHAL), FQ3F), columns, FQ3F)
    failed = debug.validate_constraints(pipeline.bitwise_air_constraints(N, LIMB_BITS), CHAL, [], trace, built, raise_on_failure=False)
    assert failed.failures == [(TRANSITION, N - 1, 1)]
    with pytest.raises(debug.ConstraintViolation) as bad:
        debug.validate_constraints(pipeline.bitwise_air_constraints(N, LIMB_BITS), CHAL, [], trace, built)
    assert (bad.value.constraint, bad.value.row) == (TRANSITION, N - 1)
    # the same flip in a trace whose limbs were NOT recomputed is seen by the recomposition of c, at that row
    cols = pipeline.bitwise_trace(N, LIMB_BITS, op, 32)
    cols[2] = c
    tampered = upload(pl, cols)
    built = build_extension_columns(pl, tampered, GpuVec.from_numpy(pl, PAIRS["fp_fq3"].ext_words(CHAL), FQ3F), columns, FQ3F)
    failed = debug.validate_constraints(pipeline.bitwise_air_constraints(N, LIMB_BITS), CHAL, [], tampered, built, raise_on_failure=False)
    assert failed.failures == [(RECOMPOSITION_C, row, 1)]
