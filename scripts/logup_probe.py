#!/usr/bin/env python3
"""One LogUp lookup column of two fractions -- `pipeline.lookup_air`'s S' = S + m / (alpha - t0 - beta t1) - 1 / (alpha - a0 - beta a1) -- over
2^20 and 2^22 rows, Fp -> Fq3, on one GPU, built three ways:
    fused     ONE ms_build_logup_columns call (three launches; the challenges read in device memory), with the time of each kernel
    product   baseline (a): ms_build_extension_columns building one running product whose map has as many terms as one denominator
              (P' = P (alpha - t0 - beta t1)) -- an entry point this column does not go through, the yardstick of what a fused builder costs
    chain     baseline (b): the entry points that existed before -- ms_fill / ms_binary / ms_binary_const materialise each denominator as an
              Fq3 column, ms_unary(MS_INV) is the InverseInto stage, ms_binary multiplies by m and adds, ms_scan_affine sums -- with the
              challenges on the host (what ms_binary_const and ms_fill take)
`fused` and `chain` must produce the same words; the script stops if they do not.

Times: after a warm-up the three ways alternate `--reps` times; reported are the medians of (i) the sum of the library's per-launch hipEvent
pairs on its stream (ms_profile_*: kernel time, by kernel for the fused call) and (ii) a host clock around the calls ending in a device
synchronise (what a caller waits).  The challenge download the chain needs first is timed on its own.  Nothing is asserted about the times.

    python scripts/logup_probe.py [--log-n 20,22] [--reps 7] [--json profiles/logup_probe.json]
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
from ministark_amd import (GL_P, GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, ExtColumn, GpuVec, Matrix, Planner, build_extension_columns,  # noqa: E402
                           build_logup_columns, gl_to_mont, pipeline)

ADD, MUL = 0, 1
NEG, INV = 0, 1
A0, A1, T0, T1, M = range(5)


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


class Chain:
    """the column from stage calls and one scan: three Fq3 temporaries, 17 launches + the scan's three"""

    def __init__(self, pl, base, n, out):
        self.pl, self.L, self.base, self.n, self.out = pl, pl.lib, base, n, out
        self.dt, self.da, self.tmp = (GpuVec(pl, n, FQ3) for _ in range(3))
        self.zero = np.zeros(3, dtype=np.uint64)
        self.minus_one = np.array([gl_to_mont(GL_P - 1), 0, 0], dtype=np.uint64)

    def _denominator(self, dst, c0, c1, alpha, minus_beta):
        """dst = alpha - base[c0] - beta base[c1]"""
        L, h, n = self.L, self.pl.handle, self.n
        L.check(L.ms_fill(h, FQ3, n, dst.ptr, minus_beta.ctypes.data))
        L.check(L.ms_binary(h, MUL, FQ3, FP, n, dst.ptr, dst.ptr, self.base.columns[c1].ptr, 0))
        L.check(L.ms_fill(h, FQ3, n, self.tmp.ptr, self.minus_one.ctypes.data))
        L.check(L.ms_binary(h, MUL, FQ3, FP, n, self.tmp.ptr, self.tmp.ptr, self.base.columns[c0].ptr, 0))
        L.check(L.ms_binary(h, ADD, FQ3, FQ3, n, dst.ptr, dst.ptr, self.tmp.ptr, 0))
        L.check(L.ms_binary_const(h, ADD, FQ3, FQ3, n, dst.ptr, dst.ptr, alpha.ctypes.data))

    def run(self, ch):
        """ch: the challenges on the host, numpy [2, 3] Montgomery words"""
        L, h, n = self.L, self.pl.handle, self.n
        alpha = np.ascontiguousarray(ch[0])
        minus_beta = np.array([(GL_P - int(w)) % GL_P for w in ch[1]], dtype=np.uint64)
        self._denominator(self.dt, T0, T1, alpha, minus_beta)
        self._denominator(self.da, A0, A1, alpha, minus_beta)
        L.check(L.ms_unary(h, INV, FQ3, n, self.dt.ptr, self.dt.ptr, 0))                   # InverseInto: Montgomery's trick, inv(0) = 0
        L.check(L.ms_unary(h, INV, FQ3, n, self.da.ptr, self.da.ptr, 0))
        L.check(L.ms_binary(h, MUL, FQ3, FP, n, self.dt.ptr, self.dt.ptr, self.base.columns[M].ptr, 0))
        L.check(L.ms_unary(h, NEG, FQ3, n, self.da.ptr, self.da.ptr, 0))
        L.check(L.ms_binary(h, ADD, FQ3, FQ3, n, self.dt.ptr, self.dt.ptr, self.da.ptr, 0))
        L.check(L.ms_scan_affine(h, FQ3, n, None, self.dt.ptr, self.zero.ctypes.data, 0, self.out.ptr))


def profiled(pl, fn):
    """-> (sum of the kernel times in us, launches, {kernel name: us})"""
    pl.sync()
    pl.profile(True)
    fn()
    pl.sync()
    prof = pl.profile_read()
    pl.profile(False)
    return sum(v["total_us"] for v in prof.values()), sum(v["calls"] for v in prof.values()), {k: v["total_us"] for k, v in prof.items()}


def wall_us(pl, fn):
    pl.sync()
    t = time.perf_counter()
    fn()
    pl.sync()
    return (time.perf_counter() - t) * 1e6


def measure(pl, log_n, reps, rehearsal):
    n = 1 << log_n
    cols = pipeline.lookup_trace(n, 9)
    base = Matrix.from_numpy(pl, [pipeline.to_mont_words(FP, c).ravel() for c in cols], FP)
    rng = np.random.default_rng(10)
    chal = GpuVec.from_numpy(pl, rng.integers(0, GL_P, size=6, dtype=np.uint64), FQ3)
    lookup = pipeline.lookup_air(n)[4]
    product = [ExtColumn(1, [(+1, 0, None), (-1, None, T0), (-1, 1, T1)], [])]
    fused_out, product_out, chain_out = ([GpuVec(pl, n, FQ3)] for _ in range(3))
    chain = Chain(pl, base, n, chain_out[0])
    ch = chal.to_numpy().reshape(-1, 3)
    ways = (("fused", lambda: build_logup_columns(pl, base, chal, lookup, FQ3, out=fused_out)),
            ("product", lambda: build_extension_columns(pl, base, chal, product, FQ3, out=product_out)),
            ("chain", lambda: chain.run(ch)))
    for _, fn in ways:                                                  # warm-up, and: faster and different is not faster
        fn()
    if not np.array_equal(fused_out[0].to_numpy(), chain_out[0].to_numpy()):
        raise SystemExit(f"2^{log_n} rows: the fused call and the chain disagree")
    for _, fn in ways:
        fn()
    t = {f"{name}_{what}_us": [] for name, _ in ways for what in ("kernel", "wall")}
    t["challenge_download_us"] = []
    launches, split = {}, {}
    for _ in range(reps):
        for name, fn in ways:
            us, calls, by_kernel = profiled(pl, fn)
            t[f"{name}_kernel_us"].append(us)
            launches[name] = calls
            if name == "fused":
                for k, v in by_kernel.items():
                    split.setdefault(k, []).append(v)
        for name, fn in ways:
            t[f"{name}_wall_us"].append(wall_us(pl, fn))
        t["challenge_download_us"].append(wall_us(pl, chal.to_numpy))
    if rehearsal:
        print(f"rehearsal, 2^{log_n} rows -- launches: {launches}; kernels of the fused call: {sorted(split)}; the outputs agree")
        return None
    med = {k: round(float(np.median(v)), 1) for k, v in t.items()}
    ratio = lambda a, b: round(med[a] / med[b], 3) if med[b] else None
    # what the fused call must move: five term columns read once, the Fq3 column written (increments), read and written again
    fused_bytes = 8 * n * 5 + 3 * 24 * n
    # what the chain moves at the least: every stage reads its operands and writes its result (Fq3: 24 bytes, Fp: 8), the scan reads b and writes out
    chain_bytes = n * (2 * (24 + (24 + 8 + 24) + 24 + (24 + 8 + 24) + 3 * 24 + 2 * 24) + 2 * 2 * 24 + (24 + 8 + 24) + 2 * 24 + 3 * 24 + 2 * 24)
    return {"shape": {"log_n": log_n, "columns": 1, "fractions": 2, "terms_per_denominator": 3, "reps": reps},
            "launches": launches, **med,
            "fused_kernels_us": {k: round(float(np.median(v)), 1) for k, v in sorted(split.items())},
            "all": {k: [round(x, 1) for x in v] for k, v in t.items()},
            "fused_over_chain_kernel_time": ratio("fused_kernel_us", "chain_kernel_us"),
            "fused_over_chain_wall_time": ratio("fused_wall_us", "chain_wall_us"),
            "fused_over_product_kernel_time": ratio("fused_kernel_us", "product_kernel_us"),
            "fused_algorithmic_bytes": fused_bytes, "chain_algorithmic_bytes": chain_bytes,
            "fused_algorithmic_GBps": round(fused_bytes / med["fused_kernel_us"] / 1e3, 1) if med["fused_kernel_us"] else None}


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
