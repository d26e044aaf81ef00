"""`bench.py --dump-outputs DIR` and the plain run, at toy sizes on the simulator build of the library: the line carries the contract's
keys and `steps` timed steps, a plain run measures nothing besides the headline, and the dumped columns are what W + K forward coset
transforms of the seeded inputs give by the oracle -- however many transforms the settle phase ran before them."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cref  # noqa: E402


def _run(tmp_path, args):
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    env = dict(os.environ, MS_BENCH_LIB=build_emu.build(), MS_BENCH_DIST_BACKEND="gloo", MS_BENCH_NO_PMC="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, cwd=str(tmp_path), env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_dumps_what_its_steps_computed(tmp_path):
    log_n, cols, steps, warmup = 10, 2, 3, 2
    out = tmp_path / "dump"
    line = _run(tmp_path, ["--log-n", str(log_n), "--cols", str(cols), "--steps", str(steps), "--warmup", str(warmup), "--settle", "0.2",
                           "--dump-outputs", str(out)])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0 and line["unit"] == "GB/s"
    assert "roofline" not in line and "cpu_baseline" not in line and "sharded_root" not in line     # measured with --full only
    lo, hi, pos = (np.load(out / f) for f in ("ntt_columns_lo.npy", "ntt_columns_hi.npy", "ntt_positions.npy"))
    assert lo.dtype == hi.dtype == pos.dtype == np.float64 and lo.shape == hi.shape == (cols, 1 << log_n)
    got = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    rng = np.random.default_rng(0x6D696E69)                     # bench.py's inputs of rank 0
    for c in range(cols):
        x = rng.integers(0, cref.GL_P, size=1 << log_n, dtype=np.uint64)
        for _ in range(warmup + steps):
            x = cref.ntt(x, log_n, 1, False, 7)
        assert np.array_equal(got[c], x[pos.astype(np.int64)]), c
