#!/usr/bin/env python3
"""Cost of one constraint validation (ministark_amd.debug.validate_constraints) after a warm-up, timed with the library's per-launch
events (ms_profile_*), for three AIRs:
    fib        pipeline.fib_air_constraints (17 constraints, 8 Fp columns), 2^22 rows
    running    17 Fp + 9 Fq3 columns, running-product transitions + boundaries (19 constraints, Fq3 challenges), 2^20 rows
    fib252     the fib AIR over the 252-bit field, 2^20 rows
Every trace is all zeros: each AIR then holds on every row but a few (the boundaries), the common case of a nearly right trace.
`--failing` fills the columns with random values instead (every transition fails on every row: the counting path everywhere).

    python scripts/validate_probe.py [--failing] [--json out.json]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ministark_amd import GOLDILOCKS_FP, GOLDILOCKS_FQ3, STARK252_FP, GL_P, Matrix, Planner, pipeline  # noqa: E402
from ministark_amd import expr as E  # noqa: E402
from ministark_amd.api import Radix2EvaluationDomain  # noqa: E402
from ministark_amd.debug import validate_constraints  # noqa: E402


def running_product_air(n):
    x = E.X()
    last = pow(Radix2EvaluationDomain(n, 1).group_gen, n - 1, GL_P)
    b = [lambda o=0, k=k: E.Trace(k, o) for k in range(17)]
    e = [lambda o=0, k=k: E.Trace(17 + k, o) for k in range(9)]
    zer = (x - E.Constant(last)) / (x ** n - E.Constant(1))
    cons = [(e[k](1) - e[k]() * (E.Challenge(k % 4) - b[k]() * E.Challenge((k + 1) % 4) - b[k + 8](1))) * zer for k in range(9)]
    cons += [e[k]() / (x - E.Constant(1)) for k in range(9)]
    cons.append((b[16]() ** 2 - b[16]()) * zer)
    return cons


def columns(pl, n, k, field, failing, rng):
    V = {GOLDILOCKS_FP: 1, GOLDILOCKS_FQ3: 3, STARK252_FP: 4}[field]
    if not failing:
        return Matrix.from_numpy(pl, [np.zeros(n * V, dtype=np.uint64) for _ in range(k)], field)
    cols = []
    for _ in range(k):
        c = rng.integers(0, GL_P, size=n * V, dtype=np.uint64)
        if field == STARK252_FP:
            c[3::4] >>= np.uint64(8)
        cols.append(c)
    return Matrix.from_numpy(pl, cols, field)


def main():
    failing = "--failing" in sys.argv
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    pl = Planner(0)
    rng = np.random.default_rng(7)
    ch3 = [(3, 5, 7), (11, 13, 17), (19, 23, 29), (31, 37, 41)]
    cases = [
        ("fib", 22, lambda n: (pipeline.fib_air_constraints(n), [], [5], columns(pl, n, 8, GOLDILOCKS_FP, failing, rng), None)),
        ("running", 20, lambda n: (running_product_air(n), ch3, [], columns(pl, n, 17, GOLDILOCKS_FP, failing, rng),
                                   columns(pl, n, 9, GOLDILOCKS_FQ3, failing, rng))),
        ("fib252", 20, lambda n: (pipeline.fib_air_constraints(n, STARK252_FP), [], [5], columns(pl, n, 8, STARK252_FP, failing, rng), None)),
    ]
    pl.profile(True)
    results = []
    for name, log_n, make in cases:
        n = 1 << log_n
        cons, ch, hints, base, ext = make(n)
        validate_constraints(cons, ch, hints, base, ext, raise_on_failure=False)          # warm-up: plans, pool blocks, code load
        before = pl.profile_read()                                                         # the event records accumulate: take the difference
        t0 = time.perf_counter()
        rep = validate_constraints(cons, ch, hints, base, ext, raise_on_failure=False)
        wall = (time.perf_counter() - t0) * 1e3
        after = pl.profile_read()
        kern = {k: (v["total_us"] - before.get(k, {"total_us": 0.0})["total_us"]) / 1e3 for k, v in after.items() if k.startswith("validate")}
        r = {"air": name, "rows": n, "constraints": len(cons), "trace": "random" if failing else "zeros",
             "kernel_ms": round(sum(kern.values()), 3), "per_kernel_ms": {k: round(v, 3) for k, v in kern.items()},
             "call_wall_ms": round(wall, 3), "failing_constraints": len(rep.failures)}
        print(json.dumps(r), flush=True)
        results.append(r)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
