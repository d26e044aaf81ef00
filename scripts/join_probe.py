#!/usr/bin/env python3
"""ms_join_rows -- for every row, the table row that holds its key -- on one GPU, one key set, every probe row drawn uniformly from a table
of distinct random keys, for Fp at width 1 and 2 and Fp252 at width 1:
    (a) square   n_table = n in {2^20, 2^22}: beside it ms_lookup_multiplicities on the same keys (table and looked-up columns in one
                 matrix), whose lookup_count kernel is the yardstick for join_match -- the same walk, with an atomic add where the join has
                 a store
    (b) rom      n_table in {2^8, 2^12, 2^16} against n = 2^22: the slot array is sized by the table and stays in cache.  These are the
                 numbers a table kept in LDS would have to beat.
    host         what a caller had to do before the call existed, on the Fp width 1 data of every shape: download the two key columns, index
                 on the host with numpy (argsort the table's keys, searchsorted), upload the index
The device's match array must be the index the rows were drawn by, in every entry, the report must count them all as matched, and the
host's index must be the device's; the script stops if they are not.

Times: after a warm-up the ways alternate `--reps` times; reported are the medians of (i) the library's per-launch hipEvent pairs on its
stream (ms_profile_*: kernel time, by kernel -- join_clear is the two memsets that empty the slots and zero the counters) and (ii) a host
clock around the call ending in a device synchronise (what a caller waits; for the host route the download, the indexing and the upload,
each also on its own).  Nothing is asserted about the times.

    python scripts/join_probe.py [--log-n 20,22] [--log-table 8,12,16] [--log-probe 22] [--reps 7] [--json profiles/join_probe.json]
`--lib PATH` runs the same logic against another build of the library (the simulator, at small sizes) to rehearse it; nothing is written
then, a simulator has no times.
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from ministark_amd import GL_P, GOLDILOCKS_FP as FP, STARK252_FP as FP252, DeviceIndex, GpuVec, LookupTuple, Matrix, Planner, join_rows, lookup_multiplicities  # noqa: E402

VARIANTS = (("fp_w1", FP, 1, 1), ("fp_w2", FP, 1, 2), ("fp252_w1", FP252, 4, 1))       # name, field, words per element, key width
JOIN_KERNELS = ("join_clear", "join_build", "join_match", "join_finish")
LOOKUP_KERNELS = ("lookup_clear", "lookup_build", "lookup_count", "lookup_finish")


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


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


def random_keys(rng, rows, V, width):
    """`width` columns of `rows` distinct random elements as Montgomery words -- any word below p is some value's; the top limb of an Fp252
    element is kept below 2^59, so the element is below p = 2^251 + 17 2^192 + 1"""
    cols = []
    for _ in range(width):
        if V == 1:
            cols.append(rng.integers(0, GL_P, size=rows, dtype=np.uint64))
        else:
            w = rng.integers(0, 1 << 63, size=(rows, V), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, size=(rows, V), dtype=np.uint64)
            w[:, V - 1] >>= np.uint64(5)
            cols.append(w.ravel())
    return cols


def gather(col, idx, V):
    return col.reshape(-1, V)[idx].ravel()


def host_index(table_keys, probe_keys):
    """Fp width 1 on Montgomery words (one value, one word): the row of every probe key in a table of distinct keys"""
    order = np.argsort(table_keys, kind="stable")
    pos = np.searchsorted(table_keys[order], probe_keys)
    pos[pos == len(order)] = 0
    row = order[pos]
    return np.where(table_keys[row] == probe_keys, row, 0xFFFFFFFF).astype(np.uint32)


def measure(pl, log_table, log_n, reps, rehearsal, with_lookup):
    n_table, n = 1 << log_table, 1 << log_n
    rng = np.random.default_rng([log_table, log_n])
    idx = rng.integers(0, n_table, size=n)
    calls, held, checks = [], {}, {}
    for name, field, V, width in VARIANTS:
        tkeys = random_keys(rng, n_table, V, width)
        table = Matrix.from_numpy(pl, tkeys, field)
        base = Matrix.from_numpy(pl, [gather(c, idx, V) for c in tkeys], field)
        key = LookupTuple(range(width))
        held[name] = (table, base, tkeys)
        calls.append((name, JOIN_KERNELS, lambda table=table, base=base, key=key: join_rows(pl, table, key, base, [key])))
        if with_lookup:                                                     # the yardstick: table and looked-up columns in one matrix, n_table = n
            both = Matrix(table.columns + base.columns + [GpuVec(pl, n, field)])
            tk, lk = LookupTuple(range(width)), LookupTuple(range(width, 2 * width))
            calls.append((name + "_lookup", LOOKUP_KERNELS, lambda both=both, tk=tk, lk=lk, w=width: lookup_multiplicities(pl, both, tk, [lk], out=both.columns[2 * w])))
    host_table, host_base, _ = held["fp_w1"]
    host_out = DeviceIndex(pl, n)
    parts = {}

    def host():
        t0 = time.perf_counter()
        tk, pk = host_table.columns[0].to_numpy(), host_base.columns[0].to_numpy()
        t1 = time.perf_counter()
        row = host_index(tk, pk)
        t2 = time.perf_counter()
        pl.lib.check(pl.lib.ms_upload(pl.handle, host_out.ptr, row.ctypes.data, row.nbytes))
        pl.sync()
        parts.update(download=(t1 - t0) * 1e6, index=(t2 - t1) * 1e6, upload=(time.perf_counter() - t2) * 1e6)

    want = idx.astype(np.uint32)
    for name, kernels, fn in calls:                                          # warm-up, and: faster and different is not faster
        out, report = fn()
        if kernels is JOIN_KERNELS:
            got = out[0].to_numpy()
            if not np.array_equal(got, want) or (report.matched, report.missing, report.duplicate_table_rows, report.table_active) != (n, 0, 0, n_table):
                raise SystemExit(f"2^{log_table} x 2^{log_n}, {name}: the match array is not the index the rows were drawn by ({report!r})")
        elif report.missing or report.duplicate_table_rows:
            raise SystemExit(f"2^{log_table} x 2^{log_n}, {name}: {report!r}")
    host()
    if not np.array_equal(host_out.to_numpy(), want):
        raise SystemExit(f"2^{log_table} x 2^{log_n}: the uploaded host index is not the device's")
    t = {f"{name}_{what}_us": [] for name, _, _ in calls for what in ("kernel", "wall")}
    t.update({f"host_{what}_us": [] for what in ("wall", "download", "index", "upload")})
    split, algo = {name: {} for name, _, _ in calls}, {}
    for rep in range(reps):
        print(f"2^{log_table} x 2^{log_n}: repetition {rep + 1} of {reps}", file=sys.stderr, flush=True)
        for name, _, fn in calls:
            by_kernel, algo[name] = profiled(pl, fn)
            t[f"{name}_kernel_us"].append(sum(by_kernel.values()))
            for k, v in by_kernel.items():
                split[name].setdefault(k, []).append(v)
        for name, _, fn in calls:
            t[f"{name}_wall_us"].append(wall_us(pl, fn))
        t["host_wall_us"].append(wall_us(pl, host))
        for what, us in parts.items():
            t[f"host_{what}_us"].append(us)
    if rehearsal:
        print(f"rehearsal, 2^{log_table} x 2^{log_n} -- kernels: { {name: sorted(v) for name, v in split.items()} }; every match array is the index drawn, and the host's")
        return None
    med = {k: round(float(np.median(v)), 1) for k, v in t.items()}
    res = {"shape": {"log_n_table": log_table, "log_n": log_n, "sets": 1, "reps": reps}, **med, "kernels": {}}
    for name, kernels, _ in calls:
        res["kernels"][name] = {}
        for k in kernels:
            if k not in split[name]:
                continue
            us = round(float(np.median(split[name][k])), 1)
            rows = n_table if k in ("join_build", "join_clear") else n
            res["kernels"][name][k] = {"us": us, "algorithmic_bytes_per_row": round(algo[name][k] / rows, 1),
                                       "algorithmic_GBps": round(algo[name][k] / us / 1e3, 1) if us else None}
    if with_lookup:
        for name, _, _, _ in VARIANTS:
            match, count = res["kernels"][name]["join_match"]["us"], res["kernels"][name + "_lookup"]["lookup_count"]["us"]
            res[f"{name}_join_match_over_lookup_count"] = round(match / count, 3) if count else None
    res["host_over_fp_w1_wall_time"] = round(med["host_wall_us"] / med["fp_w1_wall_us"], 3) if med["fp_w1_wall_us"] else None
    res["all"] = {k: [round(x, 1) for x in v] for k, v in t.items()}
    return res


def main():
    out_path, reps, lib_path = arg("--json"), int(arg("--reps", 7)), arg("--lib")
    square = [int(v) for v in arg("--log-n", "20,22").split(",")]
    tables, log_probe = [int(v) for v in arg("--log-table", "8,12,16").split(",")], int(arg("--log-probe", 22))
    if lib_path:
        from ministark_amd import _lib
        pl = Planner(0, _lib.Lib(lib_path))
    else:
        pl = Planner(0)
    results = {}
    for log_n in square:
        res = measure(pl, log_n, log_n, reps, bool(lib_path), True)
        if res is not None:
            results[f"square_log_n_{log_n}"] = res
    for log_table in tables:
        res = measure(pl, log_table, log_probe, reps, bool(lib_path), False)
        if res is not None:
            results[f"rom_log_table_{log_table}_log_n_{log_probe}"] = res
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
