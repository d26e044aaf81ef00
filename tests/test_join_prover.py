"""`pipeline.fetch_trace_on_device`: the base trace of `lookup_air` with its a1 column FETCHED from a program table by ms_join_rows and
ms_permute_columns and its m column counted by ms_lookup_multiplicities, all where the trace lies -- in the manner of
tests/test_lookup_prover.py, whose helpers it uses:
  - the device-built trace is the uploaded `fetch_trace` in every word;
  - debug.validate_constraints accepts it for `lookup_air`;
  - `pipeline.prove` on it gives the roots, nonce, positions and every other reported value of the proof on the host-built trace;
  - negative control: one address replaced by one that the program does not hold -- `check=True` raises LookupMissing naming that row and
    that value."""
import numpy as np
import pytest

from tests import backends
from tests.logup_ref import PAIRS
from tests.test_logup_prover import BITS, BLOWUP, FOLDING, MAXREM, NQ, SEED
from tests.test_lookup_prover import REPORTED, same
from ministark_amd import GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3F, GpuVec, LookupMissing, Matrix, build_extension_columns, debug, pipeline
from ministark_amd.api import GL_P as P

KINDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
SIZES = [pytest.param("emu", 64, id="emu"), pytest.param("hip", 1024, id="hip", marks=pytest.mark.gpu)]


def test_the_host_built_trace_is_what_its_docstring_says():
    n = 64
    addr, val = pipeline.fetch_program(n, 5)
    a0, a1, t0, t1, m = pipeline.fetch_trace(n, 5)
    assert len(addr) == n // 2 == len(set(addr)) and all(0 <= v < P for v in addr + val)
    assert t0 == addr + [addr[-1]] * (n // 2) and t1 == val + [val[-1]] * (n // 2)
    held = dict(zip(addr, val))
    assert all(a1[i] == held[a0[i]] for i in range(n))
    assert m == [a0.count(a) for a in addr] + [0] * (n // 2) and sum(m) == n and max(m) >= 2


@pytest.mark.parametrize("kind,n", SIZES)
def test_the_device_built_trace_is_the_host_built_trace(kind, n):
    pl = backends.planner(kind)
    cols = pipeline.fetch_trace(n, 90 + n)
    want = [pipeline.to_mont_words(FP, c).ravel() for c in cols]
    assert any(want[1]) and any(want[4]) and not all(want[4])
    got = pipeline.fetch_trace_on_device(pl, n, 90 + n, check=True)
    assert got.num_cols() == 5 and got.field == FP
    for c, (g, w) in enumerate(zip(got.to_numpy(), want)):
        assert np.array_equal(g, w), c
    # the trace satisfies lookup_air: the LogUp column built on it, the constraints checked on the device
    comp, ce, ncoef, nair, columns = pipeline.lookup_air(n)
    chal = [(3, 1, 4), (1, 5, 9)]
    built = build_extension_columns(pl, got, GpuVec.from_numpy(pl, PAIRS["fp_fq3"].ext_words(chal), FQ3F), columns, FQ3F)
    assert debug.validate_constraints(pipeline.lookup_air_constraints(n), chal, [], got, built).ok


@pytest.mark.gpu
def test_the_proof_on_it_is_the_proof_on_the_host_built_trace():
    pl, n = backends.planner("hip"), 1024
    comp, ce, ncoef, nair, columns = pipeline.lookup_air(n)
    prove = lambda trace: pipeline.prove(pl, trace, comp, ncoef, [], SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash="sha256", keep=True, ce_blowup=ce,
                                         fq=FQ3F, num_air_challenges=nair, extension=columns)
    host = prove(Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in pipeline.fetch_trace(n, 90 + n)], FP))
    trace = pipeline.fetch_trace_on_device(pl, n, 90 + n)
    out = prove(trace)
    for key in ("base_root", "extension_root", "composition_root", "fri_roots", "nonce", "positions"):
        assert same(out[key], host[key]), key
    for key in REPORTED:
        assert same(out[key], host[key]), key
    assert debug.validate_constraints(pipeline.lookup_air_constraints(n), out["air_challenges"], [], trace, out["ext_trace"]).ok


@pytest.mark.parametrize("kind,n", SIZES)
def test_an_address_the_program_does_not_hold_is_named(kind, n):
    pl = backends.planner(kind)
    a0 = list(pipeline.fetch_trace(n, 90 + n)[0])
    addr = pipeline.fetch_program(n, 90 + n)[0]
    row, stray = n // 3, (addr[0] + 1) % P
    assert stray not in addr
    a0[row] = stray
    with pytest.raises(LookupMissing) as err:
        pipeline.fetch_trace_on_device(pl, n, 90 + n, check=True, a0=a0)
    assert (err.value.set, err.value.row, err.value.values, err.value.missing) == (0, row, [stray], 1)
    assert f"row {row}" in str(err.value) and str(stray) in str(err.value)
    # without the check the call goes through: the fetched value of that row is zero, and the multiplicity count then misses the pair
    trace = pipeline.fetch_trace_on_device(pl, n, 90 + n, a0=a0)
    assert not trace.columns[1].to_numpy()[row]
