#!/usr/bin/env python3
"""The permutation that sorts the rows of a trace by a key of base columns -- ms_sort_rows -- over 2^20 and 2^22 rows on one GPU:
    memory     (a) Fp, two components below 2^32 (address, cycle): the shape of the brainfuck memory table
    uniform    (b) Fp, one component drawn uniformly from the field: every byte of the key varies
    memory252  (c) Fp252, the two components of (a): 64 digit positions, 8 of which vary
    equal      (d) Fp, two components, all keys equal: nothing to sort
    host       (e) what a caller has to do without the call, on the data of (a): download the two key columns, take them out of Montgomery
               form, np.lexsort, upload the permutation -- and the gather (ms_permute_columns), which both routes need
For every shape the device's permutation must be the host's stable sort of the canonical values, entry for entry, and its report the shape's;
the script stops if they are not.

Times: after a warm-up the ways alternate `--reps` times; reported are the medians of (i) the library's per-launch hipEvent pairs on its
stream (ms_profile_*: kernel time, by kernel; the launches of skipped passes are in it) and (ii) a host clock around the call ending in a
device synchronise (what a caller waits; for (e) the download, the conversion, the sort and the upload, each also on its own).  Nothing is
asserted about the times.

    python scripts/sort_probe.py [--log-n 20,22] [--reps 7] [--json profiles/sort_probe.json]
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
from ministark_amd import (F252_P, GL_P, GOLDILOCKS_FP as FP, STARK252_FP as FP252, DeviceIndex, GpuVec, Matrix, Planner, SortKey,  # noqa: E402
                           f252_to_mont_limbs, permute_columns, sort_rows)

KERNELS = ("sort_clear", "sort_prepare", "sort_decide", "sort_gather", "sort_pass_hist", "sort_pass_scan", "sort_pass_scatter", "sort_finish")
EPS = np.uint64(0xFFFFFFFF)


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def gl_from_mont(w):
    """gl::from_mont (csrc/gl.h mont_mul(w, 1)) on an array of canonical Montgomery words"""
    with np.errstate(over="ignore"):
        s = w + (w << np.uint64(32))
        bb = s - (s >> np.uint64(32)) - (s < w).astype(np.uint64)
        return np.where(bb != 0, np.uint64(GL_P) - bb, np.uint64(0))


def f252_mont_words(values):
    """small canonical integers -> Fp252 Montgomery words, 4 per element: to_mont is linear, so one table per 16-bit half"""
    values = np.asarray(values, dtype=np.uint64)
    lo = [f252_to_mont_limbs(v) for v in range(1 << 16)]
    hi = [f252_to_mont_limbs(v << 16) for v in range(1 << 16)]
    as_int = lambda limbs: sum(int(x) << (64 * k) for k, x in enumerate(limbs))
    lo_i, hi_i = [as_int(x) for x in lo], [as_int(x) for x in hi]
    out = np.empty((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        m = (lo_i[int(v) & 0xFFFF] + hi_i[int(v) >> 16]) % F252_P
        out[i] = [(m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    return out.ravel()


def profiled(pl, fn):
    """-> ({kernel name: us}, {kernel name: launches})"""
    pl.sync()
    pl.profile(True)
    fn()
    pl.sync()
    prof = pl.profile_read()
    pl.profile(False)
    return {k: v["total_us"] for k, v in prof.items()}, {k: v["calls"] for k, v in prof.items()}


def wall_us(pl, fn):
    pl.sync()
    t = time.perf_counter()
    fn()
    pl.sync()
    return (time.perf_counter() - t) * 1e6


def shapes(pl, n):
    """{name: (the base Matrix, the key, the canonical key columns most significant first, the varying bytes to expect)}"""
    rng = np.random.default_rng(13)
    addr = rng.integers(0, 1 << 16, size=n).astype(np.uint64)                  # many rows per address: the cycle breaks the ties
    cycle = rng.permutation(n).astype(np.uint64)
    nbytes = lambda col: int(np.count_nonzero([(np.bitwise_or.reduce(col ^ col[0]) >> np.uint64(8 * b)) & np.uint64(0xFF) for b in range(8)]))
    words = rng.integers(0, GL_P, size=n, dtype=np.uint64)
    canon = gl_from_mont(words)
    mont = lambda col: col * EPS                                               # v 2^64 mod p = v (2^32 - 1), below p for v < 2^32
    same = np.full(n, 77, dtype=np.uint64)
    return {"memory": (Matrix.from_numpy(pl, [mont(addr), mont(cycle)], FP), SortKey([0, 1]), [addr, cycle], nbytes(addr) + nbytes(cycle)),
            "uniform": (Matrix.from_numpy(pl, [words], FP), SortKey([0]), [canon], nbytes(canon)),
            "memory252": (Matrix.from_numpy(pl, [f252_mont_words(addr), f252_mont_words(cycle)], FP252), SortKey([0, 1]), [addr, cycle], nbytes(addr) + nbytes(cycle)),
            "equal": (Matrix.from_numpy(pl, [mont(same), mont(same)], FP), SortKey([0, 1]), [same, same], 0)}


def measure(pl, log_n, reps, rehearsal):
    n = 1 << log_n
    cases = shapes(pl, n)
    calls = [(name, lambda base=base, key=key: sort_rows(pl, base, key)) for name, (base, key, _, _) in cases.items()]
    for name, fn in calls:                                               # warm-up, and: faster and different is not faster
        perm, report = fn()
        _, _, canon, varying = cases[name]
        want = np.lexsort(tuple(reversed(canon))).astype(np.uint32)      # stable; the LAST key of lexsort is the primary one
        if not np.array_equal(perm.to_numpy(), want) or (report.active, report.varying_bytes) != (n, varying):
            raise SystemExit(f"2^{log_n} rows, {name}: the device's permutation or report {report!r} is not the host's")
    base = cases["memory"][0]
    parts, keep = {}, {}

    def host():
        t0 = time.perf_counter()
        cols = [c.to_numpy() for c in base.columns]
        t1 = time.perf_counter()
        canon = [gl_from_mont(c) for c in cols]
        t2 = time.perf_counter()
        order = np.lexsort((canon[1], canon[0])).astype(np.uint32)
        t3 = time.perf_counter()
        keep["index"] = DeviceIndex.from_numpy(pl, order)
        pl.sync()
        parts.update(download=(t1 - t0) * 1e6, from_mont=(t2 - t1) * 1e6, lexsort=(t3 - t2) * 1e6, upload=(time.perf_counter() - t3) * 1e6)

    host()
    device_perm, _ = sort_rows(pl, base, cases["memory"][1])
    if not np.array_equal(keep["index"].to_numpy(), device_perm.to_numpy()):
        raise SystemExit(f"2^{log_n} rows: the uploaded host permutation is not the device's")
    out = [GpuVec(pl, n, FP) for _ in range(2)]
    gather = lambda: permute_columns(pl, base, device_perm, out=out)
    gather()
    t = {f"{name}_{what}_us": [] for name, _ in calls for what in ("kernel", "wall")}
    t.update({f"host_{what}_us": [] for what in ("wall", "download", "from_mont", "lexsort", "upload")})
    t.update({"gather_kernel_us": [], "gather_wall_us": []})
    split, launches = {name: {} for name, _ in calls}, {}
    for rep in range(reps):
        print(f"2^{log_n} rows: repetition {rep + 1} of {reps}", file=sys.stderr, flush=True)
        for name, fn in calls:
            by_kernel, launches[name] = profiled(pl, fn)
            t[f"{name}_kernel_us"].append(sum(by_kernel.values()))
            for k, v in by_kernel.items():
                split[name].setdefault(k, []).append(v)
        t["gather_kernel_us"].append(sum(profiled(pl, gather)[0].values()))
        for name, fn in calls:
            t[f"{name}_wall_us"].append(wall_us(pl, fn))
        t["gather_wall_us"].append(wall_us(pl, gather))
        t["host_wall_us"].append(wall_us(pl, host))
        for what, us in parts.items():
            t[f"host_{what}_us"].append(us)
    if rehearsal:
        print(f"rehearsal, 2^{log_n} rows -- kernels: { {name: sorted(v) for name, v in split.items()} }; every permutation is the host's")
        return None
    med = {k: round(float(np.median(v)), 1) for k, v in t.items()}
    res = {"shape": {"log_n": log_n, "reps": reps, "varying_bytes": {name: c[3] for name, c in cases.items()}}, **med, "kernels": {}}
    for name, _ in calls:
        res["kernels"][name] = {k: {"us": round(float(np.median(split[name][k])), 1), "launches": launches[name][k]} for k in KERNELS if k in split[name]}
    passes = cases["memory"][3]
    pass_us = sum(res["kernels"]["memory"][k]["us"] for k in ("sort_pass_hist", "sort_pass_scan", "sort_pass_scatter"))
    # an executed pass reads 8 bytes a row for its histogram, reads and writes 12 for its scatter: 32 bytes a row (the launches of the
    # skipped passes are in the time, so the rate is a lower bound)
    res["memory_bytes_per_row_per_pass"] = 32
    res["memory_pass_GBps_lower_bound"] = round(32.0 * n * passes / pass_us / 1e3, 1) if pass_us else None
    ratio = lambda a, b: round(med[a] / med[b], 3) if med[b] else None
    res["host_over_memory_wall_time"] = ratio("host_wall_us", "memory_wall_us")
    res["memory252_over_memory_kernel_time"] = ratio("memory252_kernel_us", "memory_kernel_us")
    res["equal_over_memory_kernel_time"] = ratio("equal_kernel_us", "memory_kernel_us")
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
