"""The column chains of the three-pass NTT (ms_ntt.cpp: run_chains) against the oracle and against the batch launches.

A call with at least two Fp columns of a three-pass plan deals its columns round-robin to S streams; each stream runs pass 1 -> 2 -> 3 of
its columns one after the other through ONE scratch column.  The kernels and the words they work on are those of the batch launches, so
every output word equals the oracle's and the batch route's.  The switches (MS_NTT_CHAINS, MS_NTT_CHAIN_STREAMS, MS_NTT_CHAIN_MIN_LOG) are
read once per process: every setting runs in a child interpreter, which checks its outputs against `oracle.cref.ntt`, saves them, and
leaves the `[ms_ntt]` lines of MS_NTT_DEBUG on stderr -- "... columns as chains on S streams" is the route's own line.

`emu` runs the same host code and kernels under the simulator of tests/emu, `hip` on the device.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
MIN_LOG = 17

# (ncols, inverse, offset, out of place) per size: every column count (1 = no split, 5 = an uneven deal for 2 and 4 streams), both
# directions, both offsets, in place and through enqueue_to.  2^17: R = 2 (ntt2_small_mid_pass), 2^19: R = 8, 2^20: R = 16
# (ntt2_mid_pass_r); 2^24 (the radix-256 middle pass) on the device alone.
CASES = {
    17: [(1, False, 7, False), (2, True, 1, True), (3, False, 1, True), (5, True, 7, False),
         (2, False, 7, True), (3, True, 7, False), (5, False, 1, False), (1, True, 1, True)],
    19: [(1, True, 7, True), (2, False, 1, False), (3, True, 1, False), (5, False, 7, True)],
    20: [(1, False, 1, False), (2, True, 7, True), (3, False, 7, False), (5, True, 1, False)],
    24: [(2, False, 7, False)],
}


# ---- what the children run ---------------------------------------------------------------------------------------------------------------
def _setup(kind):
    sys.path.insert(0, ROOT)
    from tests import backends
    return backends.planner(kind)


def child_transforms(kind, log_n, out_path):
    """Every case of CASES[log_n]: outputs checked against the oracle word for word, then saved (one array per case)."""
    from oracle import cref
    from ministark_amd import GOLDILOCKS_FP, GpuFft, GpuIfft, GpuVec, Radix2EvaluationDomain
    pl = _setup(kind)
    n = 1 << log_n
    saved = {}
    for i, (ncols, inverse, offset, to) in enumerate(CASES[log_n]):
        os.write(2, b"[case]\n")
        cols = [cref.random_elements(n, 7000 + 16 * i + c) for c in range(ncols)]
        src = [GpuVec.from_numpy(pl, c, GOLDILOCKS_FP) for c in cols]
        dst = [GpuVec(pl, n, GOLDILOCKS_FP) for _ in cols] if to else src
        plan = (GpuIfft if inverse else GpuFft)(Radix2EvaluationDomain(n, offset), GOLDILOCKS_FP, pl)
        if to:
            plan.enqueue_to(src, dst)
        else:
            plan.enqueue(src)
        pl.sync()
        got = [d.to_numpy() for d in dst]
        for c, s, g in zip(cols, src, got):
            want = cref.ntt(c, log_n, 1, inverse, offset)
            bad = np.nonzero(want != g)[0]
            assert bad.size == 0, f"case {i}: mismatch at {bad[:8]} of {bad.size}"
            if to:
                assert np.array_equal(s.to_numpy(), c), f"case {i}: the source column must be preserved"
        saved[f"case{i}"] = np.stack(got)
        plan.close()
        for v in src + (dst if to else []):
            v.free()
    np.savez(out_path, **saved)


def child_unclaimed(kind, out_path):
    """Plans the route does not claim: Fq3 columns of a three-pass plan, two-pass sizes (2^16 the pass loop, 2^18 the two-pass kernels)."""
    from oracle import cref
    from ministark_amd import GOLDILOCKS_FP, GOLDILOCKS_FQ3, GpuFft, GpuVec, Radix2EvaluationDomain
    pl = _setup(kind)
    saved = {}
    for field, V, log_n in ((GOLDILOCKS_FQ3, 3, 17), (GOLDILOCKS_FP, 1, 16), (GOLDILOCKS_FP, 1, 18)):
        n = 1 << log_n
        cols = [cref.random_elements(n * V, 8100 + log_n + c) for c in range(2)]
        vecs = [GpuVec.from_numpy(pl, c, field) for c in cols]
        plan = GpuFft(Radix2EvaluationDomain(n, 7), field, pl)
        plan.enqueue(vecs)
        pl.sync()
        got = [v.to_numpy() for v in vecs]
        for c, g in zip(cols, got):
            assert np.array_equal(g, cref.ntt(c, log_n, V, False, 7)), (V, log_n)
        saved[f"v{V}_{log_n}"] = np.stack(got)
        plan.close()
    np.savez(out_path, **saved)


def child_profiled(kind):
    """Per-launch profiling on: the batch launches run, one per pass, and the words are the oracle's."""
    from oracle import cref
    from ministark_amd import GOLDILOCKS_FP, GpuFft, GpuVec, Radix2EvaluationDomain
    pl = _setup(kind)
    log_n, n = 20, 1 << 20
    cols = [cref.random_elements(n, 8200 + c) for c in range(3)]
    vecs = [GpuVec.from_numpy(pl, c, GOLDILOCKS_FP) for c in cols]
    plan = GpuFft(Radix2EvaluationDomain(n, 7), GOLDILOCKS_FP, pl)
    pl.profile(True)
    plan.enqueue(vecs)
    calls = {name: rec["calls"] for name, rec in pl.profile_read().items()}
    pl.profile(False)
    assert calls == {"ntt_pass1": 1, "ntt_pass2": 1, "ntt_pass3": 1}, calls
    for c, v in zip(cols, vecs):
        assert np.array_equal(v.to_numpy(), cref.ntt(c, log_n, 1, False, 7))
    plan.close()


def child_back_to_back(kind):
    """Forward, then inverse on the same columns with no sync in between: the second call's fork must come after the first call's join
    (its chains reuse the scratch columns and read what the first call's side streams wrote).  Twice, so that a chain call follows one."""
    from oracle import cref
    from ministark_amd import GOLDILOCKS_FP, GpuFft, GpuIfft, GpuVec, Radix2EvaluationDomain
    pl = _setup(kind)
    log_n, n = 17, 1 << 17
    cols = [cref.random_elements(n, 8300 + c) for c in range(3)]
    vecs = [GpuVec.from_numpy(pl, c, GOLDILOCKS_FP) for c in cols]
    dom = Radix2EvaluationDomain(n, 7)
    fwd, inv = GpuFft(dom, GOLDILOCKS_FP, pl), GpuIfft(dom, GOLDILOCKS_FP, pl)
    for _ in range(2):
        fwd.enqueue(vecs)
        inv.enqueue(vecs)
    for c, v in zip(cols, vecs):
        assert np.array_equal(v.to_numpy(), c)
    fwd.enqueue(vecs)
    for c, v in zip(cols, vecs):
        assert np.array_equal(v.to_numpy(), cref.ntt(c, log_n, 1, False, 7))
    fwd.close(); inv.close()


# ---- the parent's side -------------------------------------------------------------------------------------------------------------------
def _child(call, chains, streams=None, min_log=MIN_LOG):
    """Runs `call` (an expression on this module, imported as t) in a child interpreter under the given switches; returns its [ms_ntt] lines,
    split at the children's "[case]" marks."""
    env = dict(os.environ, MS_NTT_CHAINS="1" if chains else "0", MS_NTT_CHAIN_MIN_LOG=str(min_log), MS_NTT_DEBUG="1")
    env.pop("MS_NTT_STREAMS", None)
    env.pop("MS_NTT_CHAIN_STREAMS", None)
    if streams is not None:
        env["MS_NTT_CHAIN_STREAMS"] = str(streams)
    code = "import sys; sys.path.insert(0, %r); from tests import test_ntt_chains as t; t.%s" % (ROOT, call)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return [[ln for ln in block.splitlines() if ln.startswith("[ms_ntt]")] for block in r.stderr.split("[case]\n")]


_batch = {}


def _batch_outputs(kind, log_n, tmp_path_factory):
    """The same calls under MS_NTT_CHAINS=0, once per backend and size."""
    if (kind, log_n) not in _batch:
        path = str(tmp_path_factory.mktemp("ntt_chains") / f"batch_{kind}_{log_n}.npz")
        lines = _child("child_transforms(%r, %d, %r)" % (kind, log_n, path), chains=False)
        assert not any("chains" in ln for block in lines for ln in block)
        _batch[(kind, log_n)] = dict(np.load(path))
    return _batch[(kind, log_n)]


def _chains_against_batch(kind, log_n, streams, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ntt_chains") / f"chains_{kind}_{log_n}_{streams}.npz")
    lines = _child("child_transforms(%r, %d, %r)" % (kind, log_n, path), chains=True, streams=streams)[1:]
    assert len(lines) == len(CASES[log_n])
    for (ncols, _, _, _), block in zip(CASES[log_n], lines):     # the route ran where it applies, and only there
        claimed = [ln for ln in block if "chains" in ln]
        want = [f"[ms_ntt] log_n={log_n}: {ncols} columns as chains on {min(streams, ncols)} streams"] if ncols >= 2 else []
        assert claimed == want, block
        assert len(block) - len(claimed) == 3 * (ncols if ncols >= 2 else 1)      # a launch per pass and column / per pass
    got, want = dict(np.load(path)), _batch_outputs(kind, log_n, tmp_path_factory)
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("streams", [1, 2, 4])
@pytest.mark.parametrize("log_n", [17, 19, 20])
def test_chains_equal_oracle_and_batch(kind, log_n, streams, tmp_path_factory):
    _chains_against_batch(kind, log_n, streams, tmp_path_factory)


@pytest.mark.gpu
def test_chains_equal_oracle_and_batch_radix_256_middle_pass_hip(tmp_path_factory):
    _chains_against_batch("hip", 24, 2, tmp_path_factory)


@pytest.mark.parametrize("kind", BACKENDS)
def test_route_leaves_fq3_and_two_pass_plans_alone(kind, tmp_path):
    on, off = str(tmp_path / "on.npz"), str(tmp_path / "off.npz")
    lines_on = _child("child_unclaimed(%r, %r)" % (kind, on), chains=True, streams=2, min_log=12)
    lines_off = _child("child_unclaimed(%r, %r)" % (kind, off), chains=False, min_log=12)
    assert lines_on == lines_off and lines_on[0] and not any("chains" in ln for ln in lines_on[0])
    a, b = dict(np.load(on)), dict(np.load(off))
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("kind", BACKENDS)
def test_profiling_runs_the_batch(kind):
    lines = _child("child_profiled(%r)" % kind, chains=True, streams=2)
    assert len(lines[0]) == 3 and not any("chains" in ln for ln in lines[0]), lines


@pytest.mark.parametrize("kind", BACKENDS)
@pytest.mark.parametrize("streams", [2, 4])
def test_back_to_back_calls_without_sync(kind, streams):
    lines = _child("child_back_to_back(%r)" % kind, chains=True, streams=streams)
    assert sum("chains" in ln for ln in lines[0]) == 5, lines
