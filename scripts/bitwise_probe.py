#!/usr/bin/env python3
"""Bitwise-operation columns (include/ministark_hip_bitwise.h) on one GPU, 2^22 rows: which counting form of ms_bitwise_multiplicities is
the default where, and what the call saves.

Shapes -- limbs of 4 and of 8 bits (pair tables of 2^8 and 2^16 rows, one op), 4 limbs an operand, 1 and 8 sets of distinct operand
columns, two operand shapes:
    uniform      every operand drawn uniformly below 2^(4 bits)
    skewed       half of all operands 0, the others uniform: the limb pairs (0, y), (x, 0) and (0, 0) are hot
For each shape, in one process on the same columns:
    plain        MS_BITWISE_FORM=plain: one global add per limb pair, merged per wave
    lds          MS_BITWISE_FORM=lds: a histogram per workgroup in LDS
    route        what a caller had before: ms_limb_decompose of c, then ms_lookup_multiplicities at width 4 over the limb-column tuples
                 (op, a_j, b_j, c_j) against the uploaded table -- at most 8 tuples a call, so 8 sets are four calls, whose four m columns
                 the caller would still have to add (not timed).  The limb columns of a and b are there already: the AIR has them.
Every m is compared with numpy, in every word, before anything is timed; the script stops if one differs.

Times: after a warm-up the calls of a shape alternate `--reps` times; reported are the medians of the library's per-launch hipEvent pairs
on its stream (ms_profile_*: kernel time, summed over the call's launches) and of a host clock around the call ending in a device
synchronise, with the smallest and largest kernel time beside the median.  Nothing is asserted about the times.

    python scripts/bitwise_probe.py [--log-n 22] [--reps 7] [--out profiles/bitwise_probe.txt]
`--lib PATH` runs the same logic against another build of the library (the simulator, at a small --log-n) to rehearse it."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from ministark_amd import (GOLDILOCKS_FP as FP, BitwiseSet, BitwiseSpec, GpuVec, LimbSpec, LookupTuple, Matrix, Planner, bitwise_columns,  # noqa: E402
                           bitwise_multiplicities, bitwise_table, limb_decompose, lookup_multiplicities)

EPS = np.uint64(0xFFFFFFFF)                                               # x 2^64 mod p = x (2^32 - 1), below p for x < 2^32
NLIMBS, OP = 4, "xor"


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def profiled(pl, fn):
    pl.sync()
    pl.profile(True)
    fn()
    pl.sync()
    prof = pl.profile_read()
    pl.profile(False)
    return {k: v["total_us"] for k, v in prof.items()}


def wall_us(pl, fn):
    pl.sync()
    t = time.perf_counter()
    fn()
    pl.sync()
    return (time.perf_counter() - t) * 1e6


def with_form(form, fn):
    def run():
        os.environ["MS_BITWISE_FORM"] = form                              # read by the library at every call
        try:
            return fn()
        finally:
            del os.environ["MS_BITWISE_FORM"]
    return run


def timed(pl, calls, reps):
    """calls: [(name, fn)] -> {name: (median kernel us, min, max, median wall us, {kernel: median us})} over `reps` alternating repetitions"""
    kernel, wall, split = {n: [] for n, _ in calls}, {n: [] for n, _ in calls}, {n: {} for n, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            by_kernel = profiled(pl, fn)
            kernel[name].append(sum(by_kernel.values()))
            for k, v in by_kernel.items():
                split[name].setdefault(k, []).append(v)
        for name, fn in calls:
            wall[name].append(wall_us(pl, fn))
    med = lambda v: float(np.median(v))
    return {name: (med(kernel[name]), min(kernel[name]), max(kernel[name]), med(wall[name]), {k: med(v) for k, v in split[name].items()}) for name, _ in calls}


def operands(rng, n, total, shape):
    v = rng.integers(0, 1 << total, size=n, dtype=np.uint64)
    if shape == "skewed":
        v[rng.integers(0, 2, size=n) == 0] = 0
    return v


def measure(pl, log_n, reps, bits, shape, nsets, lines):
    n, total, lm = 1 << log_n, NLIMBS * bits, np.uint64((1 << bits) - 1)
    T = 1 << (2 * bits)
    rng = np.random.default_rng([bits, len(shape), nsets])
    ab = [operands(rng, n, total, shape) for _ in range(2 * nsets)]
    # per set s: a, b, c at 3 s .. 3 s + 2; then per set the 12 limb columns a_j, b_j, c_j; then op, top, tx, ty, tz
    zero = np.zeros(n, dtype=np.uint64)
    word_cols = [w for s in range(nsets) for w in (ab[2 * s] * EPS, ab[2 * s + 1] * EPS, zero)]
    L0 = 3 * nsets
    X = L0 + 12 * nsets
    trace = Matrix.from_numpy(pl, word_cols + [zero] * (12 * nsets) + [np.full(n, 2, dtype=np.uint64) * EPS] + [zero] * 4, FP)
    bitwise_columns(pl, trace, [BitwiseSpec(OP, 3 * s, 3 * s + 1, 3 * s + 2, total) for s in range(nsets)]).check()
    limb_decompose(pl, trace, [LimbSpec(3 * s + w, L0 + 12 * s + 4 * w, NLIMBS, bits) for s in range(nsets) for w in range(3)]).check()
    bitwise_table(pl, FP, bits, [OP], n_t=n, out=trace.columns[X + 1:X + 5])
    want = np.zeros(n, dtype=np.int64)
    for s in range(nsets):
        for j in range(NLIMBS):
            sh = np.uint64(bits * j)
            want[:T] += np.bincount(((((ab[2 * s] >> sh) & lm) << np.uint64(bits)) | ((ab[2 * s + 1] >> sh) & lm)).astype(np.int64), minlength=T)
    want = want.astype(np.uint64) * EPS
    sets = [BitwiseSet(OP, 3 * s, 3 * s + 1, 3 * s + 2, NLIMBS) for s in range(nsets)]
    m = {name: GpuVec(pl, n, FP) for name in ("plain", "lds")}
    m_route = [GpuVec(pl, n, FP) for _ in range((nsets * NLIMBS + 7) // 8)]
    tuples = [LookupTuple([X, L0 + 12 * s + j, L0 + 12 * s + 4 + j, L0 + 12 * s + 8 + j]) for s in range(nsets) for j in range(NLIMBS)]
    c_specs = [LimbSpec(3 * s + 2, L0 + 12 * s + 8, NLIMBS, bits) for s in range(nsets)]

    def route():
        limb_decompose(pl, trace, c_specs)
        reports = [lookup_multiplicities(pl, trace, LookupTuple([X + 1, X + 2, X + 3, X + 4]), tuples[8 * k:8 * k + 8], out=m_route[k])[1] for k in range(len(m_route))]
        return reports

    calls = [("plain", with_form("plain", lambda: bitwise_multiplicities(pl, trace, bits, [OP], sets, out=m["plain"]))),
             ("lds", with_form("lds", lambda: bitwise_multiplicities(pl, trace, bits, [OP], sets, out=m["lds"]))),
             ("route", route)]
    for name, fn in calls[:2]:                                            # warm-up, and: faster and different is not faster
        _, report = fn()
        if not np.array_equal(m[name].to_numpy(), want) or report.missing:
            raise SystemExit(f"bits {bits}, {shape}, {nsets} sets, {name}: the device's m is not numpy's")
    reports = route()
    got = sum((v.to_numpy() // EPS).astype(np.int64) for v in m_route)                               # exact: every word is count * EPS
    if not np.array_equal(got.astype(np.uint64) * EPS, want) or any(r.missing for r in reports):
        raise SystemExit(f"bits {bits}, {shape}, {nsets} sets, route: the device's m is not numpy's")
    res = timed(pl, calls, reps)
    print(f"bits {bits}, {shape}, {nsets} set(s): done", file=sys.stderr, flush=True)
    r = res["route"][0]
    for name in ("plain", "lds", "route"):
        k_med, k_min, k_max, w_med, split = res[name]
        parts = ", ".join(f"{k} {v:.1f}" for k, v in sorted(split.items(), key=lambda kv: -kv[1])[:3])
        lines.append(f"{bits:4d}  {shape:8s} {nsets:4d}  {name:6s} {k_med:10.1f} {k_min:10.1f} {k_max:10.1f} {w_med:10.1f}  {k_med / r if r else 0.0:8.4f}   {parts}")     # r = 0: a simulator has no times
    return res


def main():
    out_path, reps, lib_path, log_n = arg("--out"), int(arg("--reps", 7)), arg("--lib"), int(arg("--log-n", 22))
    if lib_path:
        from ministark_amd import _lib
        pl = Planner(0, _lib.Lib(lib_path))
    else:
        pl = Planner(0)
    lines = [f"ms_bitwise_multiplicities, 2^{log_n} rows, {NLIMBS} limbs an operand, op {OP}, one op slot; medians of {reps} alternated repetitions in one process",
             "kernel us: the sum of the call's launches by the library's per-launch events; wall us: a host clock around the call, ending in a synchronise",
             "route: ms_limb_decompose of c + ms_lookup_multiplicities at width 4 over the limb-column tuples against the uploaded table (8 tuples a call)",
             "",
             "bits  shape    sets  form    kernel us        min        max    wall us  /route     the call's three longest launches (us)"]
    for bits in (4, 8):
        for shape in ("uniform", "skewed"):
            for nsets in (1, 8):
                measure(pl, log_n, reps, bits, shape, nsets, lines)
    text = "\n".join(lines) + "\n"
    if lib_path:
        print("rehearsal against", lib_path, "-- every result is numpy's; no times on a simulator, nothing written")
        return
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
