#!/usr/bin/env python3
"""The first FRI layer of a proof over the 252-bit field, by the two routes the library offers, on one GPU: 8 columns of 2^20 rows
(random canonical elements: the work does not depend on the trace being valid), blow-up 4, every column opened at z and g z, one
composition column.
    (i)  ms_deep_compose (coset transforms of every polynomial, the composition, an inverse transform, the degree adjustment), then
         the LDE of the result with its bit reversal                        DeepPolyComposer.into_deep_poly + into_bit_reversed_evaluations
    (ii) ms_deep_rows on the rows of the committed LDEs                    DeepPolyComposer.into_deep_evaluations
After a warm-up the two are alternated `--reps` times; each run is timed by the library's per-launch hipEvents on its stream (the sum
over the launches of the route) and by a host clock that ends in a device synchronise; medians are reported, and the words are compared.
Then the whole proof (pipeline.prove_phases, field=STARK252_FP, folding 8) with its phase split, SHA-256 and BLAKE2s alternated.

    python scripts/deep252_probe.py [--log-rows 20] [--reps 5] [--json out.json]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ministark_amd import STARK252_FP as F, Matrix, Planner, Radix2EvaluationDomain, pipeline  # noqa: E402
from ministark_amd.api import F252_P  # noqa: E402
from ministark_amd.composer import DeepPolyComposer  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def random_column(rng, n):
    w = rng.integers(0, 2 ** 64, size=(n, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64(2 ** 59 - 1)                    # below 2^251 < p: four canonical words
    return w.ravel()


def kernels(pl, fn):
    pl.sync()
    pl.profile(True)
    out = fn()
    pl.sync()
    prof = pl.profile_read()
    pl.profile(False)
    return out, {k: round(v["total_us"], 1) for k, v in prof.items()}


def wall_ms(pl, fn):
    pl.sync()
    t = time.perf_counter()
    fn()
    pl.sync()
    return (time.perf_counter() - t) * 1e3


def main():
    log_t, reps = arg("--log-rows", 20), arg("--reps", 5)
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    blowup, folding, ncols = 4, 8, 8
    n, N = 1 << log_t, (1 << log_t) * blowup
    pl = Planner(0)
    rng = np.random.default_rng(252)
    trace = Matrix.from_numpy(pl, [random_column(rng, n) for _ in range(ncols)], F)
    comp, ce, nch = pipeline.fib_constraints(n, ncols, F)
    draws = pipeline.Draws(9, ncols, nch, ce, 32, N, pipeline.fri_num_layers(N, blowup, folding, 64), modulus=F252_P)
    lde_dom = Radix2EvaluationDomain(N, 3, F)
    base_polys = trace.interpolate(Radix2EvaluationDomain(n, 1, F))
    comp_polys = Matrix.from_numpy(pl, [random_column(rng, n)], F)
    base_lde, comp_lde = base_polys.bit_reversed_evaluate(lde_dom), comp_polys.bit_reversed_evaluate(lde_dom)
    composer = DeepPolyComposer(draws.trace_args, n, draws.z, base_polys, None, comp_polys)
    composer.get_ood_evals()
    routes = {
        "i_compose_then_lde": lambda: Matrix([composer.into_deep_poly(draws.deep)]).into_bit_reversed_evaluations(lde_dom).columns[0],
        "ii_deep_rows": lambda: composer.into_deep_evaluations(draws.deep, base_lde, None, comp_lde, N),
    }
    words = {k: fn().to_numpy() for k, fn in routes.items()}                  # warm-up (plans, tables) and the comparison
    res = {"shape": f"{ncols} columns x 2^{log_t} rows, blow-up {blowup}, {len(draws.trace_args) + 1} terms, 2 points", "reps": reps,
           "same_words": bool(np.array_equal(words["i_compose_then_lde"], words["ii_deep_rows"]))}
    del words
    ev = {k: [] for k in routes}
    wl = {k: [] for k in routes}
    last = {}
    for _ in range(reps):
        for k, fn in routes.items():
            _, prof = kernels(pl, fn)
            ev[k].append(sum(prof.values()))
            last[k] = prof
            wl[k].append(wall_ms(pl, fn))
    for k in routes:
        res[k] = {"kernels_us_median": round(float(np.median(ev[k])), 1), "kernels_us_all": [round(x, 1) for x in ev[k]],
                  "wall_ms_median": round(float(np.median(wl[k])), 3), "launches_us": last[k]}
    res["ii_over_i_kernel_time"] = round(res["ii_deep_rows"]["kernels_us_median"] / res["i_compose_then_lde"]["kernels_us_median"], 3)
    del base_lde, comp_lde, base_polys, comp_polys, composer

    def prove(h):
        return pipeline.prove_phases(pl, trace, comp, draws, blowup, folding, 64, 8, hash=h, ce_blowup=ce, field=F)
    hashes = ("sha256", "blake2s")
    for h in hashes:
        prove(h)
    runs = {h: [] for h in hashes}
    for _ in range(reps):
        for h in hashes:
            runs[h].append(prove(h)["phases_ms"])
    for h in hashes:
        phases = {k: round(float(np.median([r[k] for r in runs[h]])), 3) for k in runs[h][0]}
        res[f"prove_{h}"] = {"total_ms_median": round(float(np.median([sum(r.values()) for r in runs[h]])), 3), "phases_ms_median": phases}
    print(json.dumps(res, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
