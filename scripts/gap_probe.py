#!/usr/bin/env python3
"""A memory table derived where the processor table lies -- ms_gap_plan and ms_gap_fill -- over 2^20 and 2^22 processor rows on one GPU,
over Fp and Fp252.  The processor table has the memory-table shape: columns cycle, mp, mem_val, instr of a tape machine whose pointer drifts
to the right (70 % of the instructions change the cell, 25 % move right, 5 % move left), so an address is revisited a few times at short
distances and the derived table has about twice the rows; the last row has instr 0.  The rows are ordered by ms_sort_rows (not timed here:
scripts/sort_probe.py), then:
    plan       ms_gap_plan through the permutation: group mp, counter cycle, mask instr != 0
    fill       ms_gap_fill: cycle as a counter, mp and mem_val as copies, dummy as a flag, to the least power of two
    gather     ms_permute_columns gathering four columns to the same number of rows through an index that names, for every output row,
               the source row ms_gap_fill takes it from -- the yardstick for "streams as a gather streams", in the same run
    host       (Fp only) what a caller has to do without the calls: download the four columns, take mp and cycle out of Montgomery form,
               filter, np.lexsort, insert the dummy rows and pad with numpy, put cycle and dummy back into Montgomery form, upload
The device's table must be the host's in every word, and its report the host's counts; the script stops if they are not.

Times: after a warm-up the ways alternate `--reps` times; reported are the medians of (i) the library's per-launch hipEvent pairs on its
stream (ms_profile_*: kernel time, by kernel) and (ii) a host clock around the call ending in a device synchronise.  The fill's and the
gather's rates count the bytes they must move: per output row and column an element read and an element written, plus the 8 bytes of
start[] (the 4 of the index) per output row and column.  Nothing is asserted about the times.

    python scripts/gap_probe.py [--log-n 20,22] [--reps 7] [--json profiles/gap_probe.json]
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
from ministark_amd import (F252_P, GL_P, GOLDILOCKS_FP as FP, STARK252_FP as FP252, DeviceIndex, GapSpec, GpuVec, Matrix, Planner, SortKey,  # noqa: E402
                           f252_to_mont_limbs, gap_fill, gap_plan, permute_columns, sort_rows)

EPS = np.uint64(0xFFFFFFFF)
COLUMNS = [("counter", 0), ("copy", 1), ("copy", 2), ("flag", None)]
M64 = 0xFFFFFFFFFFFFFFFF


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def gl_from_mont(w):
    """gl::from_mont (csrc/gl.h mont_mul(w, 1)) on an array of canonical Montgomery words"""
    with np.errstate(over="ignore"):
        s = w + (w << np.uint64(32))
        bb = s - (s >> np.uint64(32)) - (s < w).astype(np.uint64)
        return np.where(bb != 0, np.uint64(GL_P) - bb, np.uint64(0))


_F252_TABLES = []


def f252_mont_words(values):
    """canonical integers below 2^32 -> Fp252 Montgomery words, 4 per element.  to_mont is linear: one table per 16-bit half, the two
    entries added limb by limb with carries and p subtracted once where the sum reaches it, on whole arrays."""
    values = np.asarray(values, dtype=np.uint64)
    if not _F252_TABLES:
        _F252_TABLES.append(np.array([f252_to_mont_limbs(v) for v in range(1 << 16)], dtype=np.uint64))
        _F252_TABLES.append(np.array([f252_to_mont_limbs(v << 16) for v in range(1 << 16)], dtype=np.uint64))
    a, b = _F252_TABLES[0][(values & np.uint64(0xFFFF)).astype(np.int64)], _F252_TABLES[1][(values >> np.uint64(16)).astype(np.int64)]
    p = [np.uint64((F252_P >> (64 * k)) & M64) for k in range(4)]
    out = np.empty((len(values), 4), dtype=np.uint64)
    with np.errstate(over="ignore"):
        carry = np.zeros(len(values), dtype=np.uint64)
        for k in range(4):                                                     # a + b < 2p < 2^253: no carry out of the top limb
            s = a[:, k] + b[:, k]
            c1 = s < a[:, k]
            t = s + carry
            c2 = t < s
            out[:, k] = t
            carry = (c1 | c2).astype(np.uint64)
        ge = np.ones(len(values), dtype=bool)                                  # out >= p, decided from the top limb down
        decided = np.zeros(len(values), dtype=bool)
        for k in (3, 2, 1, 0):
            gt, lt = out[:, k] > p[k], out[:, k] < p[k]
            ge = np.where(~decided & lt, False, ge)
            decided |= gt | lt
        borrow = np.zeros(len(values), dtype=np.uint64)
        for k in range(4):
            d = out[:, k] - p[k]
            b1 = out[:, k] < p[k]
            e = d - borrow
            b2 = d < borrow
            out[:, k] = np.where(ge, e, out[:, k])
            borrow = (b1 | b2).astype(np.uint64)
    return out.ravel()


def processor_rows(n, seed=13):
    """-> cycle, mp, mem_val, instr as uint64 arrays of canonical values below 2^32.  mem_val is the magnitude of the cell's value before
    the instruction (the probe moves it, it does not prove with it)."""
    rng = np.random.default_rng(seed)
    instr = rng.choice(np.array([1, 2, 3, 4], dtype=np.int64), size=n, p=[0.35, 0.35, 0.25, 0.05])
    instr[-1] = 0
    move = np.where(instr == 3, 1, np.where(instr == 4, -1, 0))
    walk = np.concatenate(([0], np.cumsum(move)[:-1]))                         # the pointer BEFORE the instruction, were there no wall
    mp = walk - np.minimum(np.minimum.accumulate(walk), 0)                     # left at address 0 stays
    delta = np.where(instr == 1, 1, np.where(instr == 2, -1, 0))
    order = np.lexsort((np.arange(n), mp))
    run = np.cumsum(delta[order]) - delta[order]                               # exclusive, along the rows of an address
    first = np.concatenate(([True], mp[order][1:] != mp[order][:-1]))
    run -= run[np.maximum.accumulate(np.where(first, np.arange(n), 0))]        # minus its value at the address's first row
    val = np.empty(n, dtype=np.int64)
    val[order] = np.abs(run)
    return [np.arange(n, dtype=np.uint64), mp.astype(np.uint64), val.astype(np.uint64), instr.astype(np.uint64)]


def derive(cycle, mp, val, instr):
    """the host derivation on canonical arrays -> (cycle, mp, mem_val, dummy of the padded table, the source row of every output row,
    the counts of the report)"""
    keep = np.nonzero(instr != 0)[0]
    order = keep[np.lexsort((cycle[keep], mp[keep]))]
    c, a = cycle[order].astype(np.int64), mp[order]
    gap = np.zeros(len(order), dtype=np.int64)
    same = a[1:] == a[:-1]
    gap[:-1] = np.where(same, c[1:] - c[:-1] - 1, 0)
    cnt = 1 + gap
    rows_out = int(cnt.sum())
    n_out = 1
    while n_out < rows_out:
        n_out *= 2
    cnt[-1] += n_out - rows_out                                                # the padding continues the last row
    src = np.repeat(np.arange(len(order)), cnt)
    k = np.arange(n_out) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    report = {"active": len(order), "rows_out": rows_out, "gaps": int(np.count_nonzero(gap)), "max_gap": int(gap.max()), "unordered": 0, "saturated": 0}
    return (c[src] + k).astype(np.uint64), a[src], val[order][src], (k > 0).astype(np.uint64), order[src].astype(np.uint32), report


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


def measure(pl, log_n, reps, rehearsal):
    n = 1 << log_n
    canon = processor_rows(n)
    want = derive(*canon)
    n_out, report = len(want[0]), want[5]
    mont = {"fp": (lambda col: col * EPS), "fp252": f252_mont_words}           # v 2^64 mod p = v (2^32 - 1), below p for v < 2^32
    field = {"fp": FP, "fp252": FP252}
    spec, key = GapSpec(group=[1], counter=0, mask=("nonzero", 3)), SortKey([1, 0], mask=("nonzero", 3))
    state, calls = {}, []
    for name in ("fp", "fp252"):
        base = Matrix.from_numpy(pl, [mont[name](c) for c in canon], field[name])
        perm, _ = sort_rows(pl, base, key)
        plan = gap_plan(pl, base, spec, perm=perm)
        got = {k: getattr(plan.report, k) for k in report}
        if got != report or plan.report.first_unordered is not None:
            raise SystemExit(f"2^{log_n} rows, {name}: the device's report {plan.report!r} is not the host's {report}")
        out = [GpuVec(pl, n_out, field[name]) for _ in COLUMNS]
        table = gap_fill(pl, base, plan, COLUMNS)
        if table.num_rows() != n_out:
            raise SystemExit(f"2^{log_n} rows, {name}: {table.num_rows()} rows for {n_out}")
        for c, w in enumerate(want[:4]):                                       # faster and different is not faster
            if not np.array_equal(table.columns[c].to_numpy(), mont[name](w)):
                raise SystemExit(f"2^{log_n} rows, {name}: column {c} of the device's table is not the host's")
        del table
        index = DeviceIndex.from_numpy(pl, want[4])
        state[name] = (base, perm, plan, out, index)
        calls.append((f"{name}_plan", lambda base=base, perm=perm: gap_plan(pl, base, spec, perm=perm)))
        calls.append((f"{name}_fill", lambda base=base, plan=plan, out=out: gap_fill(pl, base, plan, COLUMNS, n_out=n_out, out=out)))
        calls.append((f"{name}_gather", lambda base=base, index=index, out=out: permute_columns(pl, base, index, out=out)))
    base = state["fp"][0]
    parts, keep = {}, {}

    def host():
        t0 = time.perf_counter()
        cols = [c.to_numpy() for c in base.columns]
        t1 = time.perf_counter()
        cyc, mp = gl_from_mont(cols[0]), gl_from_mont(cols[1])
        t2 = time.perf_counter()
        c, a, v, d, _, _ = derive(cyc, mp, cols[2], cols[3])                   # mem_val is only moved: its words stay as they are
        t3 = time.perf_counter()
        words = [c * EPS, a * EPS, v, d * EPS]
        t4 = time.perf_counter()
        keep["table"] = Matrix.from_numpy(pl, words, FP)
        pl.sync()
        parts.update(download=(t1 - t0) * 1e6, from_mont=(t2 - t1) * 1e6, derive=(t3 - t2) * 1e6, to_mont=(t4 - t3) * 1e6, upload=(time.perf_counter() - t4) * 1e6)

    host()
    device = gap_fill(pl, base, state["fp"][2], COLUMNS)
    for c in range(4):
        if not np.array_equal(keep["table"].columns[c].to_numpy(), device.columns[c].to_numpy()):
            raise SystemExit(f"2^{log_n} rows: column {c} of the uploaded host table is not the device's")
    del device
    t = {f"{name}_{what}_us": [] for name, _ in calls for what in ("kernel", "wall")}
    t.update({f"host_{what}_us": [] for what in ("wall", "download", "from_mont", "derive", "to_mont", "upload")})
    split = {name: {} for name, _ in calls}
    for rep in range(reps):
        print(f"2^{log_n} rows: repetition {rep + 1} of {reps}", file=sys.stderr, flush=True)
        for name, fn in calls:
            by_kernel = profiled(pl, fn)
            t[f"{name}_kernel_us"].append(sum(by_kernel.values()))
            for k, v in by_kernel.items():
                split[name].setdefault(k, []).append(v)
        for name, fn in calls:
            t[f"{name}_wall_us"].append(wall_us(pl, fn))
        t["host_wall_us"].append(wall_us(pl, host))
        for what, us in parts.items():
            t[f"host_{what}_us"].append(us)
    if rehearsal:
        print(f"rehearsal, 2^{log_n} rows -> {n_out}: kernels { {name: sorted(v) for name, v in split.items()} }; every table is the host's; report {report}")
        return None
    med = {k: round(float(np.median(v)), 1) for k, v in t.items()}
    res = {"shape": {"log_n": log_n, "reps": reps, "n_out": n_out, **report}, **med, "kernels": {}}
    for name, _ in calls:
        res["kernels"][name] = {k: round(float(np.median(v)), 1) for k, v in split[name].items()}
    for name, V in (("fp", 1), ("fp252", 4)):
        fill_bytes, gather_bytes = (16.0 * V + 8.0) * n_out * 4, (16.0 * V + 4.0) * n_out * 4
        res[f"{name}_fill_GBps"] = round(fill_bytes / med[f"{name}_fill_kernel_us"] / 1e3, 1) if med[f"{name}_fill_kernel_us"] else None
        res[f"{name}_gather_GBps"] = round(gather_bytes / med[f"{name}_gather_kernel_us"] / 1e3, 1) if med[f"{name}_gather_kernel_us"] else None
        res[f"{name}_fill_over_gather_kernel_time"] = round(med[f"{name}_fill_kernel_us"] / med[f"{name}_gather_kernel_us"], 3) if med[f"{name}_gather_kernel_us"] else None
    device_wall = med["fp_plan_wall_us"] + med["fp_fill_wall_us"]
    res["host_over_device_wall_time"] = round(med["host_wall_us"] / device_wall, 1) if device_wall else None
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
