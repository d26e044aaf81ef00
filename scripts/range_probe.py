#!/usr/bin/env python3
"""Range-check columns (include/ministark_hip_range.h) on one GPU, 2^22 rows.

Counts -- ms_range_multiplicities over 1 and 8 looked-up columns, tables of 2^8, 2^12, 2^16 and 2^20 rows, three value shapes:
    uniform      every row drawn uniformly from the table
    zero         every row 0: one counter takes every add
    high         half the rows 0, half uniform: the high limb of a trace of mostly small values
in each counting form (MS_RANGE_FORM=plain: one global add per row, merged per wave; lds: a histogram per workgroup in LDS, bits <= 16),
and beside each, in the same run on the same columns, the route a caller had before: ms_lookup_multiplicities at width 1 against the
column t[j] = min(j, 2^bits - 1).
Decomposition -- ms_limb_decompose over Fp at (bits, nlimbs) = (16, 4) and (1, 64) and over Fp252 at (32, 8), as bytes moved per second
(the source and every limb column, once each), and beside it ms_unary (negation) over the same number of bytes: the streaming rate of
scripts/stage_probe.py.
Every result is compared with numpy, in every word, before anything is timed; the script stops if one differs.

Times: after a warm-up the calls of a shape alternate `--reps` times; reported are the medians of the library's per-launch hipEvent pairs
on its stream (ms_profile_*: kernel time, by kernel), and of a host clock around the call ending in a device synchronise.  Nothing is
asserted about the times.

    python scripts/range_probe.py [--log-n 22] [--reps 7] [--json profiles/range_probe.json]
`--lib PATH` runs the same logic against another build of the library (the simulator, at a small --log-n) to rehearse it; nothing is
written then, a simulator has no times.
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from ministark_amd import (F252_P, GL_P, GOLDILOCKS_FP as FP, STARK252_FP as FP252, GpuVec, LimbSpec, LookupTuple, Matrix, Planner, RangeSet,  # noqa: E402
                           f252_to_mont_limbs, limb_decompose, lookup_multiplicities, range_multiplicities)

EPS = np.uint64(0xFFFFFFFF)                                               # c 2^64 mod p = c (2^32 - 1), below p for c < 2^32
MS_NEG = 0


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def profiled(pl, fn):
    """-> {kernel name: us}"""
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
        os.environ["MS_RANGE_FORM"] = form                                # read by the library at every call
        try:
            return fn()
        finally:
            del os.environ["MS_RANGE_FORM"]
    return run


def timed(pl, calls, reps, label):
    """calls: [(name, fn)] -> {name: {"kernel_us", "wall_us", "kernels": {kernel: us}}}, medians over `reps` alternating repetitions"""
    kernel, wall, split = {n: [] for n, _ in calls}, {n: [] for n, _ in calls}, {n: {} for n, _ in calls}
    for rep in range(reps):
        for name, fn in calls:
            by_kernel = profiled(pl, fn)
            kernel[name].append(sum(by_kernel.values()))
            for k, v in by_kernel.items():
                split[name].setdefault(k, []).append(v)
        for name, fn in calls:
            wall[name].append(wall_us(pl, fn))
    print(f"{label}: {reps} repetitions", file=sys.stderr, flush=True)
    med = lambda v: round(float(np.median(v)), 1)
    return {name: {"kernel_us": med(kernel[name]), "wall_us": med(wall[name]), "kernels": {k: med(v) for k, v in split[name].items()}} for name, _ in calls}


def draw(rng, n, bits, shape):
    if shape == "zero":
        return np.zeros(n, dtype=np.uint64)
    v = rng.integers(0, 1 << bits, size=n, dtype=np.uint64)
    if shape == "high":
        v[rng.integers(0, 2, size=n) == 0] = 0
    return v


def measure_counts(pl, log_n, reps, rehearsal):
    n, out = 1 << log_n, {}
    for bits in (8, 12, 16, 20):
        if (1 << bits) > n:
            continue
        table = np.minimum(np.arange(n, dtype=np.uint64), np.uint64((1 << bits) - 1)) * EPS
        for shape in ("uniform", "zero", "high"):
            rng = np.random.default_rng([bits, len(shape)])
            vals = [draw(rng, n, bits, shape) for _ in range(8)]
            trace = Matrix.from_numpy(pl, [v * EPS for v in vals] + [table], FP)
            for nsets in (1, 8):
                want = np.zeros(n, dtype=np.uint64)
                want[:1 << bits] = sum(np.bincount(v.astype(np.int64), minlength=1 << bits) for v in vals[:nsets]).astype(np.uint64)
                want *= EPS
                m = {name: GpuVec(pl, n, FP) for name in ("plain", "lds", "lookup")}
                sets = [RangeSet(c) for c in range(nsets)]
                calls = [("plain", with_form("plain", lambda: range_multiplicities(pl, trace, bits, sets, out=m["plain"])))]
                if bits <= 16:
                    calls.append(("lds", with_form("lds", lambda: range_multiplicities(pl, trace, bits, sets, out=m["lds"]))))
                calls.append(("lookup", lambda: lookup_multiplicities(pl, trace, LookupTuple([8]), [LookupTuple([c]) for c in range(nsets)], out=m["lookup"])))
                for name, fn in calls:                                    # warm-up, and: faster and different is not faster
                    _, report = fn()
                    if not np.array_equal(m[name].to_numpy(), want) or report.missing:
                        raise SystemExit(f"bits {bits}, {shape}, {nsets} sets, {name}: the device's m is not numpy's")
                res = timed(pl, calls, reps, f"counts: bits {bits}, {shape}, {nsets} set(s)")
                if rehearsal:
                    continue
                count = {name: sum(us for k, us in res[name]["kernels"].items() if k in ("range_count_plain", "range_count_lds", "lookup_build", "lookup_count")) for name in res}
                res["count_kernel_plain_over_lookup_route"] = round(res["plain"]["kernel_us"] / res["lookup"]["kernel_us"], 3)
                if "lds" in res:
                    res["count_kernel_lds_over_plain"] = round(count["lds"] / count["plain"], 3) if count["plain"] else None
                    res["count_kernel_lds_over_lookup_route"] = round(res["lds"]["kernel_us"] / res["lookup"]["kernel_us"], 3)
                out[f"bits_{bits}_{shape}_sets_{nsets}"] = res
    return out


def mont252_words(vals):
    return np.array([w for v in vals for w in f252_to_mont_limbs(v)], dtype=np.uint64)


def measure_limbs(pl, log_n, reps, rehearsal):
    n, out = 1 << log_n, {}
    rng = np.random.default_rng(5)
    for fname, field, V, bits, nlimbs in (("fp", FP, 1, 16, 4), ("fp", FP, 1, 1, 64), ("fp252", FP252, 4, 32, 8)):
        # 2^14 distinct values, repeated down the column: the Montgomery form of 4 M values on Python integers is minutes, and a streaming
        # kernel does not see the repetition
        tile = min(n, 1 << 14)
        if V == 1:
            vals = [int(x) for x in rng.integers(0, 1 << 63, size=tile, dtype=np.uint64)]
            words = lambda xs: np.array([(x << 64) % GL_P for x in xs], dtype=np.uint64)
        else:
            vals = [int.from_bytes(rng.bytes(32), "little") >> 5 for _ in range(tile)]
            assert all(x < F252_P for x in vals)
            words = mont252_words
        src = np.tile(words(vals), n // tile)
        want = [np.tile(words([(x >> (bits * j)) & ((1 << bits) - 1) for x in vals]), n // tile) for j in range(nlimbs)]
        cols = [GpuVec.from_numpy(pl, src, field)] + [GpuVec(pl, n, field) for _ in range(nlimbs)]
        specs = [LimbSpec(0, 1, nlimbs, bits)]
        moved = (1 + nlimbs) * n * 8 * V
        a, b = GpuVec(pl, moved // 16, FP), GpuVec(pl, moved // 16, FP)    # the unary stage reads and writes 8 bytes per element
        L = pl.lib
        calls = [("limb_decompose", lambda: limb_decompose(pl, cols, specs)),
                 ("ms_unary", lambda: L.check(L.ms_unary(pl.handle, MS_NEG, FP, moved // 16, b.ptr, a.ptr, 0)))]
        report = calls[0][1]()
        calls[1][1]()
        if report.overflow or report.active != n or any(not np.array_equal(c.to_numpy(), w) for c, w in zip(cols[1:], want)):
            raise SystemExit(f"{fname} ({bits}, {nlimbs}): the device's limbs are not numpy's")
        res = timed(pl, calls, reps, f"limbs: {fname} ({bits}, {nlimbs})")
        if rehearsal:
            continue
        us = res["limb_decompose"]["kernels"]["limb_decompose"]
        res["bytes_moved"] = moved
        res["limb_decompose_GBps"] = round(moved / us / 1e3, 1)
        res["ms_unary_GBps"] = round(moved / res["ms_unary"]["kernel_us"] / 1e3, 1)
        res["limb_decompose_over_ms_unary_time"] = round(us / res["ms_unary"]["kernel_us"], 3)
        out[f"{fname}_bits_{bits}_limbs_{nlimbs}"] = res
    return out


def main():
    out_path, reps, lib_path, log_n = arg("--json"), int(arg("--reps", 7)), arg("--lib"), int(arg("--log-n", 22))
    if lib_path:
        from ministark_amd import _lib
        pl = Planner(0, _lib.Lib(lib_path))
    else:
        pl = Planner(0)
    parts = arg("--parts", "limbs,counts").split(",")
    results = {"shape": {"log_n": log_n, "reps": reps}}
    if "limbs" in parts:
        results["limbs"] = measure_limbs(pl, log_n, reps, bool(lib_path))
    if "counts" in parts:
        results["counts"] = measure_counts(pl, log_n, reps, bool(lib_path))
    if lib_path:
        print("rehearsal against", lib_path, "-- every result is numpy's; no times on a simulator, nothing written")
        return
    print(json.dumps(results, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"timing": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
