#!/usr/bin/env python3
"""Nine Fq3 extension columns of the brainfuck AIR's shapes (examples/brainfuck/trace.rs:108-289) over 2^22 rows, built two ways on one GPU:
    fused   ONE ms_build_extension_columns call (three launches; the challenges read in device memory)
    chain   the entry points that existed before it -- ms_convert / ms_binary_const / ms_binary per term, ms_fill, then ms_scan_affine per
            column -- with the challenges on the host (what ms_binary_const takes).  This is the yardstick.
The columns: four 3-term products P' = P (a - b x - c y) under a padding mask, three running evaluations E' = d E + x, two unmasked 2-term
products.  The mask column holds 0 / 1, so that the chain can express "inactive rows are the identity map" with stage calls
(a := 1 + m (a - 1)).  Both ways must produce the same words; the script stops if they do not.

Times: after a warm-up the two ways alternate `--reps` times; reported are the medians of (i) the sum of the library's per-launch hipEvent
pairs on its stream (ms_profile_*: kernel time) and (ii) a host clock around the calls ending in a device synchronise (what a caller waits).
The challenge download the chain needs first is timed on its own.

    python scripts/ext_columns_probe.py [--log-n 22] [--reps 7] [--json profiles/ext_columns_probe.json]
    python scripts/ext_columns_probe.py --resources --json profiles/ext_columns_probe.json     # no GPU: registers / LDS from the assembly
`--json` updates the named file: the two modes fill different keys of it.  `--lib PATH` runs the timing mode's logic against another build of
the library (the simulator, at a small --log-n) to rehearse it; nothing is written then, a simulator has no times.
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from ministark_amd import GL_P, GOLDILOCKS_FP as FP, GOLDILOCKS_FQ3 as FQ3, ExtColumn, GpuVec, Matrix, Planner, build_extension_columns, gl_to_mont  # noqa: E402

ADD, MUL = 0, 1
NBASE, MASK = 17, 16                       # the brainfuck AIR's 17 base columns; the last one is the 0 / 1 padding indicator here
NCHAL = 11


def columns():
    product3 = lambda a, b, c, x, y: ExtColumn(1, [(+1, a, None), (-1, b, x), (-1, c, y)], [], mask=("nonzero", MASK))
    evaluation = lambda d, x: ExtColumn(0, [(+1, d, None)], [(+1, None, x)])
    product2 = lambda a, b, x: ExtColumn(1, [(+1, a, None), (-1, b, x)], [])
    return ([product3(0, 1, 2, 0, 1), product3(0, 3, 4, 2, 3), product3(5, 6, 7, 4, 5), product3(5, 8, 9, 6, 7)] +
            [evaluation(10, 8), evaluation(10, 9), evaluation(3, 10)] + [product2(0, 1, 11), product2(5, 6, 12)])


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def update_json(path, section):
    data = json.load(open(path)) if path and os.path.exists(path) else {}
    data.update(section)
    if path:
        with open(path, "w") as f:
            json.dump(data, f, indent=1)
            f.write("\n")
    print(json.dumps(section, indent=1))


# ---- registers, scratch and LDS of the fused kernels, from the gfx950 assembly (scripts/kernel_resources.py for one unit) ----------------
def resources(out_path):
    import isa_count
    import kernel_resources
    from ministark_amd import build as msbuild
    msbuild.embed_headers()
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = kernel_resources.listing(os.path.join(msbuild.CSRC, "ms_ext.cpp"), tmp)
        md = isa_count.meta(path)
        names = [n for n, _ in isa_count.kernels(path) if n in md]
        dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        for name, d in zip(names, dem):
            m = md[name]
            rows[d.split("(")[0].replace("void ", "")] = {
                "vgpr": m.get("vgpr_count", 0), "sgpr": m.get("sgpr_count", 0), "scratch_bytes": m.get("private_segment_fixed_size", 0),
                "lds_bytes": m.get("group_segment_fixed_size", 0), "vgpr_spills": m.get("vgpr_spill_count", 0)}
    update_json(out_path, {"kernel_resources": rows})


# ---- the unfused chain ----------------------------------------------------------------------------------------------------------------------
class Chain:
    def __init__(self, pl, base, n, outs):
        self.pl, self.L, self.base, self.n, self.outs = pl, pl.lib, base, n, outs
        self.t1, self.t2, self.b = (GpuVec(pl, n, FQ3) for _ in range(3))
        self.one = np.array([gl_to_mont(1), 0, 0], dtype=np.uint64)
        self.minus_one = np.array([gl_to_mont(GL_P - 1), 0, 0], dtype=np.uint64)
        self.zero = np.zeros(3, dtype=np.uint64)

    def _scaled(self, dst, col, coef):
        """dst = coef * base[col] (coef: Fq3 words on the host)"""
        L, h, n = self.L, self.pl.handle, self.n
        L.check(L.ms_convert(h, FQ3, FP, n, dst.ptr, self.base.columns[col].ptr))
        L.check(L.ms_binary_const(h, MUL, FQ3, FQ3, n, dst.ptr, dst.ptr, coef.ctypes.data))

    def run(self, cols, ch):
        """ch: the challenges on the host, numpy [NCHAL, 3] Montgomery words; -ch their negations"""
        L, h, n = self.L, self.pl.handle, self.n
        neg = np.array([[(GL_P - int(w)) % GL_P for w in row] for row in ch], dtype=np.uint64)
        coef = lambda sign, k: np.ascontiguousarray(ch[k] if sign > 0 else neg[k])
        for c, out in zip(cols, self.outs):
            init = self.one if c.init == 1 else self.zero
            if c.b_terms:                                             # a running evaluation: a = d everywhere, b = x
                (_, d, _), (_, _, x) = c.a_terms[0][:3], c.b_terms[0][:3]
                L.check(L.ms_fill(h, FQ3, n, self.t1.ptr, coef(+1, d).ctypes.data))
                L.check(L.ms_convert(h, FQ3, FP, n, self.b.ptr, self.base.columns[x].ptr))
                L.check(L.ms_scan_affine(h, FQ3, n, self.t1.ptr, self.b.ptr, init.ctypes.data, 0, out.ptr))
                continue
            const, *terms = c.a_terms                                 # a product: a = const + sum of scaled columns
            self._scaled(self.t1, terms[0][2], coef(terms[0][0], terms[0][1]))
            for t in terms[1:]:
                self._scaled(self.t2, t[2], coef(t[0], t[1]))
                L.check(L.ms_binary(h, ADD, FQ3, FQ3, n, self.t1.ptr, self.t1.ptr, self.t2.ptr, 0))
            if c.mask is None:
                L.check(L.ms_binary_const(h, ADD, FQ3, FQ3, n, self.t1.ptr, self.t1.ptr, coef(const[0], const[1]).ctypes.data))
            else:                                                     # a := 1 + m (a - 1) with the 0 / 1 indicator column
                shifted = np.ascontiguousarray(coef(const[0], const[1]).copy())
                shifted[0] = (int(shifted[0]) + int(self.minus_one[0])) % GL_P
                L.check(L.ms_binary_const(h, ADD, FQ3, FQ3, n, self.t1.ptr, self.t1.ptr, shifted.ctypes.data))
                L.check(L.ms_binary(h, MUL, FQ3, FP, n, self.t1.ptr, self.t1.ptr, self.base.columns[c.mask[1]].ptr, 0))
                L.check(L.ms_binary_const(h, ADD, FQ3, FQ3, n, self.t1.ptr, self.t1.ptr, self.one.ctypes.data))
            L.check(L.ms_scan_affine(h, FQ3, n, self.t1.ptr, None, init.ctypes.data, 0, out.ptr))


def kernel_us(pl, fn):
    pl.sync()
    pl.profile(True)
    fn()
    pl.sync()
    prof = pl.profile_read()
    pl.profile(False)
    return sum(v["total_us"] for v in prof.values()), sum(v["calls"] for v in prof.values())


def wall_us(pl, fn):
    pl.sync()
    t = time.perf_counter()
    fn()
    pl.sync()
    return (time.perf_counter() - t) * 1e6


def main():
    out_path = arg("--json")
    if "--resources" in sys.argv:
        return resources(out_path)
    log_n, reps, lib_path = int(arg("--log-n", 22)), int(arg("--reps", 7)), arg("--lib")
    if lib_path:
        from ministark_amd import _lib
        pl = Planner(0, _lib.Lib(lib_path))
    else:
        pl = Planner(0)
    n = 1 << log_n
    rng = np.random.default_rng(9)
    base = Matrix.from_numpy(pl, [rng.integers(0, GL_P, size=n, dtype=np.uint64) for _ in range(NBASE - 1)] +
                             [np.where(rng.integers(0, 8, size=n) > 0, np.uint64(gl_to_mont(1)), np.uint64(0)).astype(np.uint64)])
    chal = GpuVec.from_numpy(pl, rng.integers(0, GL_P, size=3 * NCHAL, dtype=np.uint64), FQ3)
    cols = columns()
    fused_out = [GpuVec(pl, n, FQ3) for _ in cols]
    chain_out = [GpuVec(pl, n, FQ3) for _ in cols]
    chain = Chain(pl, base, n, chain_out)
    ch = chal.to_numpy().reshape(-1, 3)
    fused = lambda: build_extension_columns(pl, base, chal, cols, FQ3, out=fused_out)
    unfused = lambda: chain.run(cols, ch)
    fused(); unfused()                                                 # warm-up, and: faster and different is not faster
    for k, (a, b) in enumerate(zip(fused_out, chain_out)):
        if not np.array_equal(a.to_numpy(), b.to_numpy()):
            raise SystemExit(f"column {k}: the fused call and the chain disagree")
    fused(); unfused()
    t = {"fused_kernel_us": [], "chain_kernel_us": [], "fused_wall_us": [], "chain_wall_us": [], "challenge_download_us": []}
    launches = {}
    for _ in range(reps):
        for name, fn in (("fused", fused), ("chain", unfused)):
            us, calls = kernel_us(pl, fn)
            t[f"{name}_kernel_us"].append(us)
            launches[name] = calls
        for name, fn in (("fused", fused), ("chain", unfused)):
            t[f"{name}_wall_us"].append(wall_us(pl, fn))
        t["challenge_download_us"].append(wall_us(pl, chal.to_numpy))
    med = {k: round(float(np.median(v)), 1) for k, v in t.items()}
    nterm_cols = sum(sum(1 for x in c.a_terms + c.b_terms if x[2] is not None) + (c.mask is not None) for c in cols)
    res = {"shape": {"log_n": log_n, "columns": len(cols), "reps": reps, "base_column_reads_per_pass": nterm_cols},
           "launches": launches, **med, "all": {k: [round(x, 1) for x in v] for k, v in t.items()},
           "fused_over_chain_kernel_time": round(med["fused_kernel_us"] / med["chain_kernel_us"], 3) if med["chain_kernel_us"] else None,
           # what the fused kernels must move: every term / mask column read twice (aggregate and apply passes), every output written once
           "fused_algorithmic_bytes": 2 * 8 * n * nterm_cols + 24 * n * len(cols)}
    res["fused_algorithmic_GBps"] = round(res["fused_algorithmic_bytes"] / med["fused_kernel_us"] / 1e3, 1) if med["fused_kernel_us"] else None
    if lib_path:
        print("rehearsal against", lib_path, "-- launches:", launches, "; the outputs agree; no times on a simulator, nothing written")
        return
    update_json(out_path, {"timing": res})


if __name__ == "__main__":
    main()
