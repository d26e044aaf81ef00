#!/usr/bin/env python3
"""What the canonical-form scan and checked mode cost on the device (profiles/README.md).

    python scripts/canon_probe.py [--reps 5] [--log-rows 24] [--out FILE]

One JSON line per field: ms_check_canonical over 8 columns of 2^log-rows elements in one call against eight ms_unary(MS_NEG) calls into
disjoint destinations over the same buffers (the negation moves twice the bytes) -- kernel time from the library's per-launch events
(ms_profile_*), median of `reps`, the two alternated, after a warm-up.  Then one line for prove_phases at configs[4]'s shape (2^22 rows x 8
columns, blow-up 4, folding 8): wall time with checked mode off and on, alternated, and the scans' share of the kernel time."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ministark_amd import GL_P, GOLDILOCKS_FP, GOLDILOCKS_FQ3, STARK252_FP, GpuVec, Matrix, Planner, api, pipeline  # noqa: E402

WORDS = {GOLDILOCKS_FP: 1, GOLDILOCKS_FQ3: 3, STARK252_FP: 4}
NAMES = {GOLDILOCKS_FP: "fp", GOLDILOCKS_FQ3: "fq3", STARK252_FP: "fp252"}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def kernel_us(pl, fn, name):
    pl.sync()
    pl.profile(True)
    fn()
    us = pl.profile_read()[name]["total_us"]
    pl.profile(False)
    return us


def column(rng, field, n):
    if field == STARK252_FP:
        a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        a[:, 3] >>= np.uint64(6)                                  # below 2^250: canonical
        return a
    a = rng.integers(0, GL_P, size=n * WORDS[field], dtype=np.uint64)
    return a.reshape(n, 3) if field == GOLDILOCKS_FQ3 else a


def main():
    reps, log_rows, out_path = arg("--reps", 5), arg("--log-rows", 24), arg("--out", "")
    pl = Planner(0)
    rng = np.random.default_rng(9)
    lines = []
    for field in (GOLDILOCKS_FP, GOLDILOCKS_FQ3, STARK252_FP):
        n, ncols = 1 << log_rows, 8
        src = [GpuVec.from_numpy(pl, column(rng, field, n), field) for _ in range(ncols)]
        dst = [GpuVec(pl, n, field) for _ in range(ncols)]

        def scan():
            assert api.check_canonical(pl, src).count == 0

        def neg():
            for s, d in zip(src, dst):
                pl.lib.check(pl.lib.ms_unary(pl.handle, 0, field, n, d.ptr, s.ptr, 0))
        for _ in range(2):
            scan()
            neg()
        ts, tn = [], []
        for _ in range(reps):
            ts.append(kernel_us(pl, scan, "canon_scan"))
            tn.append(kernel_us(pl, neg, "stage_neg"))
        s, g = float(np.median(ts)), float(np.median(tn))
        nbytes = 8.0 * WORDS[field] * n * ncols
        lines.append({"what": "scan_vs_neg", "field": NAMES[field], "cols": ncols, "log_rows": log_rows, "bytes_read": nbytes, "canon_scan_us": round(s, 1),
                      "scan_TBps": round(nbytes / s / 1e6, 3), "neg8_us": round(g, 1), "neg_TBps_moved": round(2 * nbytes / g / 1e6, 3),
                      "scan_over_neg": round(s / g, 3), "reps": reps})
        print(json.dumps(lines[-1]), flush=True)
        del src, dst
    # prove_phases at configs[4]'s shape, checked off and on
    log_t, blowup, folding, ncols = 22, 4, 8, 8
    n_t = 1 << log_t
    trace = Matrix.from_numpy(pl, [rng.integers(0, GL_P, size=n_t, dtype=np.uint64) for _ in range(ncols)])
    comp, ce, nch = pipeline.fib_constraints(n_t, ncols)
    draws = pipeline.Draws(7, ncols, nch, ce, 32, n_t * blowup, pipeline.fri_num_layers(n_t * blowup, blowup, folding, 64))

    def prove():
        return pipeline.prove_phases(pl, trace, comp, draws, blowup, folding, 64, 8, ce_blowup=ce, time_phases=False)

    def wall(on):
        pl.checked(on)
        pl.sync()
        t = time.perf_counter()
        prove()
        pl.sync()
        return (time.perf_counter() - t) * 1e3
    for on in (False, True):
        wall(on)
    ms = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):
            ms[on].append(wall(on))
    pl.checked(True)
    pl.sync()
    pl.profile(True)
    prove()
    prof = pl.profile_read()
    pl.profile(False)
    pl.checked(False)
    lines.append({"what": "prove_phases_configs4", "log_rows": log_t, "cols": ncols, "blowup": blowup, "folding": folding,
                  "unchecked_ms": round(float(np.median(ms[False])), 3), "checked_ms": round(float(np.median(ms[True])), 3),
                  "checked_over_unchecked": round(float(np.median(ms[True]) / np.median(ms[False])), 3),
                  "scans": prof["canon_scan"]["calls"], "scan_kernels_us": round(prof["canon_scan"]["total_us"] + prof["canon_fold"]["total_us"], 1),
                  "all_kernels_us": round(sum(v["total_us"] for v in prof.values()), 1), "reps": reps})
    print(json.dumps(lines[-1]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
