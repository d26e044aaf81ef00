#!/usr/bin/env python3
"""The m column of a lookup -- how often each row of a table of pairs (t0, t1) is looked up by the pairs (a0, a1) -- over 2^20 and 2^22 rows,
Fp, width 2, one set, on one GPU:
    uniform      (a) ms_lookup_multiplicities on a table of distinct random pairs, every lookup row drawn uniformly from it
    sequential   (b) the same call on the table (j, j): keys 0 .. n-1 in both components, lookups drawn uniformly
    one_row      (c) the same call with EVERY lookup row holding the pair of one table row: one 32-bit counter takes n atomic adds
    uniform_plain, one_row_plain   (a) and (c) with one atomicAdd per lookup row (MS_LOOKUP_PLAIN_ADDS=1) in place of the library's one add per
                 wave for the lanes that found the same row as the wave's first finder -- the form the library had first
    host         (d) what a caller had to do before the call existed, on the data of (a): download the four key columns, count on the host with
                 numpy (ONE np.unique over a structured view of table and lookups, first occurrences, np.bincount), upload m
The device's m must be what the shape was built to give, in every word, and the host's count on (a) must be the device's; the script
stops if they are not.

Times: after a warm-up the four ways alternate `--reps` times; reported are the medians of (i) the library's per-launch hipEvent pairs on
its stream (ms_profile_*: kernel time, by kernel -- lookup_clear is the two memsets that empty the slots and zero the counters) and (ii) a
host clock around the call ending in a device synchronise (what a caller waits; for (d) the download, the count and the upload, each also
on its own).  Nothing is asserted about the times.

    python scripts/lookup_probe.py [--log-n 20,22] [--reps 7] [--json profiles/lookup_probe.json]
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
from ministark_amd import GL_P, GOLDILOCKS_FP as FP, GpuVec, LookupTuple, Matrix, Planner, lookup_multiplicities  # noqa: E402

A0, A1, T0, T1, M = range(5)
PAIR = np.dtype([("x", np.uint64), ("y", np.uint64)])
KERNELS = ("lookup_clear", "lookup_build", "lookup_count", "lookup_finish")


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def host_count(a0, a1, t0, t1):
    """the loop of include/ministark_hip_lookup.h in numpy, on Montgomery words (one value, one word) -> m as Montgomery words"""
    n = len(t0)
    both = np.empty(2 * n, dtype=PAIR)
    both["x"][:n], both["y"][:n], both["x"][n:], both["y"][n:] = t0, t1, a0, a1
    _, first, inverse = np.unique(both, return_index=True, return_inverse=True)
    row = first[inverse.ravel()[n:]]                                     # the first record holding a lookup's pair: a table row if below n
    cnt = np.bincount(row[row < n], minlength=n).astype(np.uint64)
    return cnt * np.uint64(0xFFFFFFFF)                                   # c 2^64 mod p = c (2^32 - 1), below p for c < 2^32


def profiled(pl, fn):
    """-> ({kernel name: us}, {kernel name: algorithmic bytes})"""
    pl.sync()
    pl.profile(True)
    fn()
    pl.sync()
    prof = pl.profile_read()
    pl.profile(False)
    return {k: v["total_us"] for k, v in prof.items()}, {k: v["bytes_per_call"] for k, v in prof.items()}


def wall_us(pl, fn):
    pl.sync()
    t = time.perf_counter()
    fn()
    pl.sync()
    return (time.perf_counter() - t) * 1e6


def shapes(n):
    """{name: (the four key columns as Montgomery words, the counts to expect)} -- any word below p is some value's, so random words are
    random values, and 2^22 random pairs of them are distinct"""
    rng = np.random.default_rng(11)
    t = rng.integers(0, GL_P, size=(2, n), dtype=np.uint64)
    idx = rng.integers(0, n, size=n)
    seq = np.arange(n, dtype=np.uint64) * np.uint64(0xFFFFFFFF)          # 0 .. n-1 in Montgomery form
    hot = n // 3
    spread, one = np.bincount(idx, minlength=n), np.zeros(n, dtype=np.int64)
    one[hot] = n
    return {"uniform": ([t[0][idx], t[1][idx], t[0], t[1]], spread),
            "sequential": ([seq[idx], seq[idx], seq, seq], spread),
            "one_row": ([np.full(n, t[0][hot]), np.full(n, t[1][hot]), t[0], t[1]], one)}


def measure(pl, log_n, reps, rehearsal):
    n = 1 << log_n
    table, lookups = LookupTuple([T0, T1]), [LookupTuple([A0, A1])]
    traces, calls, expect = {}, [], {}
    for name, (cols, counts) in shapes(n).items():
        expect[name] = counts.astype(np.uint64) * np.uint64(0xFFFFFFFF)
        trace = Matrix.from_numpy(pl, cols + [np.zeros(n, dtype=np.uint64)], FP)
        traces[name] = trace
        calls.append((name, lambda trace=trace: lookup_multiplicities(pl, trace, table, lookups, out=trace.columns[M])))

    def plain(fn):
        def run():
            os.environ["MS_LOOKUP_PLAIN_ADDS"] = "1"                    # read by the library at every call
            try:
                return fn()
            finally:
                del os.environ["MS_LOOKUP_PLAIN_ADDS"]
        return run
    for name in ("uniform", "one_row"):
        traces[name + "_plain"], expect[name + "_plain"] = traces[name], expect[name]
        calls.append((name + "_plain", plain(dict(calls)[name])))
    host_trace = traces["uniform"]
    host_m = GpuVec(pl, n, FP)
    parts = {}

    def host():
        t0 = time.perf_counter()
        keys = [host_trace.columns[c].to_numpy() for c in (A0, A1, T0, T1)]
        t1 = time.perf_counter()
        m = host_count(*keys)
        t2 = time.perf_counter()
        pl.lib.check(pl.lib.ms_upload(pl.handle, host_m.ptr, m.ctypes.data, m.nbytes))
        pl.sync()
        parts.update(download=(t1 - t0) * 1e6, count=(t2 - t1) * 1e6, upload=(time.perf_counter() - t2) * 1e6)

    for name, fn in calls:                                               # warm-up, and: faster and different is not faster
        _, report = fn()
        if not np.array_equal(traces[name].columns[M].to_numpy(), expect[name]) or report.missing or report.duplicate_table_rows:
            raise SystemExit(f"2^{log_n} rows, {name}: the device's m is not the shape's")
    host()
    if not np.array_equal(host_m.to_numpy(), host_trace.columns[M].to_numpy()):
        raise SystemExit(f"2^{log_n} rows: the uploaded host count is not the device's")
    t = {f"{name}_{what}_us": [] for name, _ in calls for what in ("kernel", "wall")}
    t.update({f"host_{what}_us": [] for what in ("wall", "download", "count", "upload")})
    split, algo = {name: {} for name, _ in calls}, {}
    for rep in range(reps):
        print(f"2^{log_n} rows: repetition {rep + 1} of {reps}", file=sys.stderr, flush=True)
        for name, fn in calls:
            by_kernel, algo[name] = profiled(pl, fn)
            t[f"{name}_kernel_us"].append(sum(by_kernel.values()))
            for k, v in by_kernel.items():
                split[name].setdefault(k, []).append(v)
        for name, fn in calls:
            t[f"{name}_wall_us"].append(wall_us(pl, fn))
        t["host_wall_us"].append(wall_us(pl, host))
        for what, us in parts.items():
            t[f"host_{what}_us"].append(us)
    if rehearsal:
        print(f"rehearsal, 2^{log_n} rows -- kernels: { {name: sorted(v) for name, v in split.items()} }; m is the shape's in every one, and the host's on (a)")
        return None
    med = {k: round(float(np.median(v)), 1) for k, v in t.items()}
    res = {"shape": {"log_n": log_n, "field": "Fp", "width": 2, "sets": 1, "reps": reps}, **med, "kernels": {}}
    for name, _ in calls:
        res["kernels"][name] = {}
        for k in KERNELS:
            us = round(float(np.median(split[name][k])), 1)
            res["kernels"][name][k] = {"us": us, "algorithmic_bytes_per_row": round(algo[name][k] / n, 1),
                                       "algorithmic_GBps": round(algo[name][k] / us / 1e3, 1) if us else None}
    ratio = lambda a, b: round(med[a] / med[b], 3) if med[b] else None
    count = lambda name: res["kernels"][name]["lookup_count"]["us"]
    res["one_row_over_uniform_count_kernel"] = round(count("one_row") / count("uniform"), 3)
    res["one_row_over_uniform_count_kernel_plain"] = round(count("one_row_plain") / count("uniform_plain"), 3)
    res["wave_over_plain_count_kernel_uniform"] = round(count("uniform") / count("uniform_plain"), 3)
    res["wave_over_plain_count_kernel_one_row"] = round(count("one_row") / count("one_row_plain"), 3)
    res["host_over_uniform_wall_time"] = ratio("host_wall_us", "uniform_wall_us")
    res["all"] = {k: [round(x, 1) for x in v] for k, v in t.items()}
    return res


def main():
    out_path, reps, lib_path = arg("--json"), int(arg("--reps", 7)), arg("--lib")
    sizes = [int(v) for v in arg("--log-n", "20,22").split(",")]
    if lib_path:
        from ministark_amd import _lib
        pl = Planner(0, _lib.Lib(lib_path))
    else:
        pl = Planner(0)
    results = {}
    for log_n in sizes:
        res = measure(pl, log_n, reps, bool(lib_path))
        if res is not None:
            results[f"log_n_{log_n}"] = res
    if lib_path:
        print("rehearsal against", lib_path, "-- no times on a simulator, nothing written")
        return
    print(json.dumps(results, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"timing": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
