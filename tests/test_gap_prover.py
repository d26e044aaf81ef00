"""`pipeline.memory_table_trace_on_device`: the memory table of a small tape machine -- the processor rows whose instr is not 0, sorted by
(mp, cycle), a dummy row for every missing cycle, padded -- built by ms_sort_rows, ms_gap_plan and ms_gap_fill where the processor table
lies, in the manner of tests/test_sort_prover.py:
  - the device-built trace is the uploaded host-built `memory_table_trace` in every word;
  - debug.validate_constraints accepts it on the reference's memory-table constraints, and rejects it with one dummy cell cleared;
  - `pipeline.prove` on it gives the roots, draws, openings and every other reported value of the proof on the host-built trace."""
import numpy as np
import pytest

from tests import backends
from tests import gaps_ref
from tests.test_extension_prover import BITS, BLOWUP, FOLDING, MAXREM, NQ, SEED
from tests.test_lookup_prover import same
from ministark_amd import GOLDILOCKS_FP as FP, GapSpec, Matrix, debug, pipeline

SIZES = [pytest.param("emu", 20, id="emu-20"), pytest.param("hip", 100, id="hip-100", marks=pytest.mark.gpu), pytest.param("hip", 400, id="hip-400", marks=pytest.mark.gpu)]
REPORTED = ("base_root", "composition_root", "fri_roots", "remainder_coeffs", "nonce", "challenges", "z", "fri_alphas", "positions", "ood", "deep", "queries",
            "fri_openings", "trace_args")
SEEDS = {20: 1, 100: 1, 400: 2}


def host_trace(steps):
    return pipeline.memory_table_trace(steps, SEEDS[steps])


def test_the_host_derivation_is_the_reference_loop_of_the_tests():
    """`memory_table_trace` against tests/gaps_ref.py: the same table by another road, and a table with gaps and padding"""
    for steps in (20, 100, 400):
        proc = pipeline.memory_processor_rows(steps, SEEDS[steps])
        assert len(proc) == 4 and len(proc[0]) == steps + 1 and proc[3][-1] == 0 and all(v in (1, 2, 3, 4) for v in proc[3][:-1])
        perm = sorted((i for i in range(steps + 1) if proc[3][i]), key=lambda i: (proc[1][i], proc[0][i])) + [steps]
        start, rep = gaps_ref.plan(proc, GapSpec(group=[1], counter=0, mask=("nonzero", 3)), perm)
        cols = host_trace(steps)
        n = len(cols[0])
        assert n & (n - 1) == 0 and n // 2 < max(rep["rows_out"], 1) <= n and rep["gaps"] > 0 and rep["unordered"] == 0 and rep["active"] == steps
        assert cols == gaps_ref.fill(proc, start, [("counter", 0), ("copy", 1), ("copy", 2), ("flag", None)], n, pipeline.GL_P, perm)
        assert sum(cols[3][:rep["rows_out"]]) == rep["rows_out"] - steps and cols[3][rep["rows_out"]:] == [1] * (n - rep["rows_out"])


@pytest.mark.parametrize("kind,steps", SIZES)
def test_the_device_built_table_is_the_host_built_table(kind, steps):
    pl = backends.planner(kind)
    cols = host_trace(steps)
    got = pipeline.memory_table_trace_on_device(pl, steps, SEEDS[steps], check=True)
    assert got.num_cols() == 4 and got.field == FP and got.num_rows() == len(cols[0])
    for c, (g, w) in enumerate(zip(got.to_numpy(), cols)):
        assert np.array_equal(g, pipeline.to_mont_words(FP, w).ravel()), c


@pytest.mark.parametrize("kind,steps", SIZES)
def test_the_constraints_hold_on_it(kind, steps):
    pl = backends.planner(kind)
    trace = pipeline.memory_table_trace_on_device(pl, steps, SEEDS[steps])
    n = trace.num_rows()
    assert debug.validate_constraints(pipeline.memory_air_constraints(n), [], [], trace).ok
    # negative controls on the first dummy cell.  dummy enters the nine base constraints only as a factor -- (dummy' - 1) dummy',
    # (mp' - mp) dummy, (mem_val' - mem_val) dummy -- so a dummy cell set to 0 satisfies them all: in the reference it is the memory
    # permutation argument (an extension column, not part of this AIR) that a cleared flag breaks.  What these constraints do reject is a
    # flag that is neither 0 nor 1, and a dummy row whose value differs from the row after it.
    first = int(np.nonzero(trace.columns[3].to_numpy())[0][0])
    word = lambda v: pipeline.to_mont_words(FP, [v]).ravel()[0]

    def altered(dummy, val=None):
        w = [c.to_numpy() for c in trace.columns]
        w[3][first] = word(dummy)
        if val is not None:
            w[2][first] = word(val)
        return debug.validate_constraints(pipeline.memory_air_constraints(n), [], [], Matrix.from_numpy(pl, w, FP), raise_on_failure=False).ok
    assert altered(1) and altered(0)
    assert not altered(2) and not altered(1, val=12345)


@pytest.mark.parametrize("kind,steps", SIZES)
def test_the_proof_on_it_is_the_proof_on_the_host_built_trace(kind, steps):
    pl = backends.planner(kind)
    cols = host_trace(steps)
    comp, ce, ncoef = pipeline.memory_air(len(cols[0]))
    prove = lambda trace: pipeline.prove(pl, trace, comp, ncoef, [], SEED, BLOWUP, FOLDING, MAXREM, BITS, NQ, hash="sha256", keep=True, ce_blowup=ce)
    host = prove(Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols], FP))
    out = prove(pipeline.memory_table_trace_on_device(pl, steps, SEEDS[steps]))
    for key in REPORTED:
        assert same(out[key], host[key]), key
