"""`pipeline.lookup_trace_on_device`: the base trace of `lookup_air` with its m column counted by ms_lookup_multiplicities where the trace
lies, in the manner of tests/test_logup_prover.py, whose helpers it uses:
  - the device-built trace is the uploaded `lookup_trace` in every word;
  - `pipeline.prove` on it gives the roots, draws, openings and every other reported value of the proof on the host-built trace;
  - debug.validate_constraints passes on it;
  - negative control: one looked-up value changed to one that is not in the table.  `report.check()` names that set, row and pair -- and
    validate_constraints on the same trace fails at the LogUp transition, at the last row, where the total is not zero.  The first is the
    answer the user needs; the second is all there was before."""
import numpy as np
import pytest

from tests import backends
from tests.logup_ref import PAIRS
from tests.test_logup_prover import BITS, BLOWUP, FOLDING, MAXREM, NQ, SEED, SIZES, TRANSITION, lookup_columns, proof
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, GpuVec, LookupMissing, LookupTuple, Matrix, build_extension_columns, debug, lookup_multiplicities, pipeline
from ministark_amd.api import GL_P as P

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
REPORTED = ("base_root", "extension_root", "composition_root", "fri_roots", "remainder_coeffs", "nonce", "challenges", "air_challenges", "z",
            "fri_alphas", "positions", "ood", "deep", "queries", "fri_openings", "trace_args")


def same(a, b):
    """equality through lists, tuples, dicts, arrays and plain records"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (int, float, str, bytes, type(None))):
        return a == b
    return type(a) is type(b) and same(vars(a), vars(b))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [16, 1024])
def test_the_device_built_trace_is_the_host_built_trace(kind, n):
    pl = backends.planner(kind)
    want = [pipeline.to_mont_words(FP, c).ravel() for c in pipeline.lookup_trace(n, 70 + n)]
    assert any(want[4]) and not all(want[4])
    got = pipeline.lookup_trace_on_device(pl, n, 70 + n, check=True)
    assert got.num_cols() == 5 and got.field == FP
    for c, (g, w) in enumerate(zip(got.to_numpy(), want)):
        assert np.array_equal(g, w), c


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_the_proof_on_it_is_the_proof_on_the_host_built_trace(kind, log_t):
    pl, n = backends.planner(kind), 1 << log_t
    host = proof(kind, log_t)[0]
    trace = pipeline.lookup_trace_on_device(pl, n, 70 + log_t)
    comp, ce, ncoef, nair, columns = pipeline.lookup_air(n)
    out = pipeline.prove(pl, trace, comp, ncoef, [], SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash="sha256", keep=True, ce_blowup=ce,
                         fq=FQ3F, num_air_challenges=nair, extension=columns)
    for key in REPORTED:
        assert same(out[key], host[key]), key
    assert np.array_equal(out["ext_trace"].to_numpy()[0], host["ext_trace"].to_numpy()[0])
    report = debug.validate_constraints(pipeline.lookup_air_constraints(n), out["air_challenges"], [], trace, out["ext_trace"])
    assert report.ok


def test_same_tells_records_apart():
    class Rec:
        def __init__(self, v):
            self.v = v
    assert same({"a": [Rec(np.arange(3)), (1, b"x")]}, {"a": [Rec(np.arange(3)), (1, b"x")]})
    assert not same({"a": [Rec(np.arange(3))]}, {"a": [Rec(np.arange(1, 4))]}) and not same([1, 2], [1, 2, 3]) and not same({"a": 1}, {"b": 1})


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_a_stray_pair_is_named_by_the_report_where_the_constraints_only_fail_at_the_wrap(kind, log_t):
    pl, n = backends.planner(kind), 1 << log_t
    cols = lookup_columns(n, log_t, stray=True)                                 # row 3 looks up a pair that is not a row of the table
    trace = Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols[:4]] + [np.zeros(n, dtype=np.uint64)], FP)
    m, report = lookup_multiplicities(pl, trace, LookupTuple([2, 3]), [LookupTuple([0, 1])], out=trace.columns[4])
    assert (report.missing, report.first_missing_set, report.first_missing_row, report.duplicate_table_rows) == (1, 0, 3, 0)
    with pytest.raises(LookupMissing) as err:
        report.check()
    assert (err.value.set, err.value.row, err.value.values) == (0, 3, [cols[0][3], cols[1][3]])
    assert "set 0, row 3" in str(err.value) and str(cols[0][3]) in str(err.value) and str(cols[1][3]) in str(err.value)
    # every other row was counted: m is the honest trace's but for the row that lost a lookup
    honest = lookup_columns(n, log_t)
    j = list(zip(honest[2], honest[3])).index((honest[0][3], honest[1][3]))
    want = list(honest[4])
    want[j] -= 1
    assert np.array_equal(m.to_numpy(), pipeline.to_mont_words(FP, want).ravel())
    # what the constraints say about the same trace: the LogUp transition, at the last row
    comp, ce, ncoef, nair, columns = pipeline.lookup_air(n)
    chal = [(3, 1, 4), (1, 5, 9)]
    built = build_extension_columns(pl, trace, GpuVec.from_numpy(pl, PAIRS["fp_fq3"].ext_words(chal), FQ3F), columns, FQ3F)
    failed = debug.validate_constraints(pipeline.lookup_air_constraints(n), chal, [], trace, built, raise_on_failure=False)
    assert failed.failures == [(TRANSITION, n - 1, 1)]
    assert (cols[0][3] - 1) % P == honest[0][3]
