"""`pipeline.sorted_permutation_trace_on_device`: a base trace of `permutation_air` whose y rows are the x rows sorted by (x0, x1) --
ms_sort_rows and ms_permute_columns where the trace lies -- in the manner of tests/test_lookup_prover.py:
  - the device-built trace is the uploaded host-sorted `sorted_permutation_trace` in every word (x0 ties, so x1 decides);
  - debug.validate_constraints accepts it, on extension columns built for challenges of the test's choosing;
  - `pipeline.prove` on it gives the roots, draws, openings and every other reported value of the proof on the host-built trace."""
import numpy as np
import pytest

from tests import backends
from tests.ext_ref import PAIRS
from tests.test_extension_prover import BITS, BLOWUP, FOLDING, MAXREM, NQ, SEED
from tests.test_lookup_prover import REPORTED, same
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, GpuVec, Matrix, build_extension_columns, debug, pipeline

SIZES = [pytest.param("emu", 6, id="emu-6"), pytest.param("hip", 6, id="hip-6", marks=pytest.mark.gpu), pytest.param("hip", 10, id="hip-10", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_the_device_sorted_trace_is_the_host_sorted_trace(kind, log_t):
    pl, n = backends.planner(kind), 1 << log_t
    cols = pipeline.sorted_permutation_trace(n, 90 + log_t)
    assert len(set(cols[0][:n - 1])) < n - 1                                    # x0 ties
    assert sorted(zip(cols[0][:n - 1], cols[1][:n - 1])) == list(zip(cols[2][:n - 1], cols[3][:n - 1]))
    got = pipeline.sorted_permutation_trace_on_device(pl, n, 90 + log_t)
    assert got.num_cols() == 4 and got.field == FP and got.num_rows() == n
    for c, (g, w) in enumerate(zip(got.to_numpy(), cols)):
        assert np.array_equal(g, pipeline.to_mont_words(FP, w).ravel()), c


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_the_constraints_hold_on_it(kind, log_t):
    pl, n = backends.planner(kind), 1 << log_t
    trace = pipeline.sorted_permutation_trace_on_device(pl, n, 90 + log_t)
    chal = [(3, 1, 4), (1, 5, 9), (2, 6, 5), (3, 5, 8)]
    columns = pipeline.permutation_air(n)[4]
    built = build_extension_columns(pl, trace, GpuVec.from_numpy(pl, PAIRS["fp_fq3"].ext_words(chal), FQ3F), columns, FQ3F)
    assert debug.validate_constraints(pipeline.permutation_air_constraints(n), chal, [], trace, built).ok
    # negative control: with one y cell changed the y rows are no permutation of the x rows
    w = [c.to_numpy() for c in trace.columns]
    w[3][1] = pipeline.to_mont_words(FP, [12345]).ravel()[0]
    broken = Matrix.from_numpy(pl, w, FP)
    built = build_extension_columns(pl, broken, GpuVec.from_numpy(pl, PAIRS["fp_fq3"].ext_words(chal), FQ3F), columns, FQ3F)
    assert not debug.validate_constraints(pipeline.permutation_air_constraints(n), chal, [], broken, built, raise_on_failure=False).ok


@pytest.mark.parametrize("kind,log_t", SIZES)
def test_the_proof_on_it_is_the_proof_on_the_host_built_trace(kind, log_t):
    pl, n = backends.planner(kind), 1 << log_t
    comp, ce, ncoef, nair, columns = pipeline.permutation_air(n)
    prove = lambda trace: pipeline.prove(pl, trace, comp, ncoef, [], SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash="sha256", keep=True, ce_blowup=ce,
                                         fq=FQ3F, num_air_challenges=nair, extension=columns)
    host = prove(Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in pipeline.sorted_permutation_trace(n, 90 + log_t)], FP))
    trace = pipeline.sorted_permutation_trace_on_device(pl, n, 90 + log_t)
    out = prove(trace)
    for key in REPORTED:
        assert same(out[key], host[key]), key
    for c in range(3):
        assert np.array_equal(out["ext_trace"].to_numpy()[c], host["ext_trace"].to_numpy()[c])
    assert debug.validate_constraints(pipeline.permutation_air_constraints(n), out["air_challenges"], [], trace, out["ext_trace"]).ok
