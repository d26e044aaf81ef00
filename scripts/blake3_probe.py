#!/usr/bin/env python3
"""BLAKE3 commitments next to SHA-256 and BLAKE2s-256 on one GPU, on the same buffers in the same process, after a warm-up, timed with
the library's per-launch hipEvents on its stream (ms_profile_*) and, for whole calls, a host clock around work that ends in a device
synchronise:
    (a) the merge level: a 2^21-leaf tree, whose level launches are those of 2^20, 2^19 and 2^18 parents (the levels below are climbed
        by the subtree kernel); reported as parents per second of the `_merkle_level` launches and as the time of 2^20 parents at that rate
    (b) leaves of 8 and of 32 Fp columns x 2^22 rows               Matrix.hash_rows
    (c) a 2^22-leaf tree                                           MerkleTree(leaves)      (level launches + subtrees + top)
    (d) prove_phases at configs[4]'s shape (2^22 rows x 8 columns, blow-up 4, folding 8) for the three hashes
Each case alternates the hashes, `--reps` times, and reports the median with the smallest and largest run beside it: a difference
inside that spread is not one.

    python scripts/blake3_probe.py [--reps 7] [--json out.json]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ministark_amd import GL_P, DeviceBytes, Matrix, MerkleTree, Planner, pipeline  # noqa: E402

HASHES = ("sha256", "blake2s", "blake3_256")
PREFIX = {"sha256": "sha256", "blake2s": "blake2s", "blake3_256": "blake3"}      # of the profiled kernel names


def kernels(pl, fn):
    """run fn once with per-launch profiling -> {kernel: (calls, total_us, bytes)}"""
    pl.sync()
    pl.profile(True)
    fn()
    pl.sync()
    prof = pl.profile_read()
    pl.profile(False)
    return {k: (v["calls"], v["total_us"], v["bytes_per_call"] * v["calls"]) for k, v in prof.items()}


def wall_ms(pl, fn):
    pl.sync()
    t = time.perf_counter()
    fn()
    pl.sync()
    return (time.perf_counter() - t) * 1e3


def stats(values, digits=1):
    """median [min .. max] of repeated runs"""
    return {"median": round(float(np.median(values)), digits), "min": round(float(min(values)), digits), "max": round(float(max(values)), digits)}


def random_leaves(pl, rng, n):
    leaves = DeviceBytes(pl, n * 32)
    raw = rng.integers(0, 256, size=n * 32, dtype=np.uint8)
    pl.lib.check(pl.lib.ms_upload(pl.handle, leaves.ptr, raw.ctypes.data, n * 32))
    return leaves


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    pl = Planner(0)
    rng = np.random.default_rng(5)
    res = {h: {} for h in HASHES}

    # (a) the merge level
    n = 1 << 21
    leaves = random_leaves(pl, rng, n)
    for h in HASHES:
        MerkleTree(pl, leaves, n, h)
    rate = {h: [] for h in HASHES}
    for _ in range(reps):
        for h in HASHES:
            calls, us, _ = kernels(pl, lambda: MerkleTree(pl, leaves, n, h))[f"{PREFIX[h]}_merkle_level"]
            assert calls == 3                                                          # 2^20, 2^19 and 2^18 parents
            rate[h].append((n - (n >> 3)) / us)                                        # parents per microsecond
    for h in HASHES:
        res[h]["merge_level_Gparents_per_s"] = stats([r / 1e3 for r in rate[h]], 3)
        res[h]["merge_level_us_per_2^20_parents"] = stats([(1 << 20) / r for r in rate[h]])
    del leaves

    # (b) leaves
    n = 1 << 22
    for ncols in (8, 32):
        m = Matrix.from_numpy(pl, [rng.integers(0, GL_P, size=n, dtype=np.uint64) for _ in range(ncols)])
        for h in HASHES:
            m.hash_rows(h)
        us = {h: [] for h in HASHES}
        for _ in range(reps):
            for h in HASHES:
                k = kernels(pl, lambda: m.hash_rows(h))
                us[h].append(sum(t for name, (c, t, b) in k.items() if name.endswith("_rows")))
        for h in HASHES:
            res[h][f"leaves_{ncols}x2^22_us"] = stats(us[h])
        del m

    # (c) a 2^22-leaf tree
    leaves = random_leaves(pl, rng, n)
    for h in HASHES:
        MerkleTree(pl, leaves, n, h)
    per = {h: {"kernels_us": [], "wall_ms": []} for h in HASHES}
    for _ in range(reps):
        for h in HASHES:
            per[h]["kernels_us"].append(sum(t for c, t, b in kernels(pl, lambda: MerkleTree(pl, leaves, n, h)).values()))
            per[h]["wall_ms"].append(wall_ms(pl, lambda: MerkleTree(pl, leaves, n, h)))
    for h in HASHES:
        res[h]["tree_2^22_kernels_us"] = stats(per[h]["kernels_us"])
        res[h]["tree_2^22_wall_ms"] = stats(per[h]["wall_ms"], 3)
    del leaves

    # (d) prove_phases at configs[4]'s shape
    log_t, blowup, folding, ncols = 22, 4, 8, 8
    n_t = 1 << log_t
    trace = Matrix.from_numpy(pl, [rng.integers(0, GL_P, size=n_t, dtype=np.uint64) for _ in range(ncols)])
    comp, ce, nch = pipeline.fib_constraints(n_t, ncols)
    nlayers = pipeline.fri_num_layers(n_t * blowup, blowup, folding, 64)
    draws = pipeline.Draws(7, ncols, nch, ce, 32, n_t * blowup, nlayers)

    def prove(h):
        return pipeline.prove_phases(pl, trace, comp, draws, blowup, folding, 64, 8, hash=h, ce_blowup=ce, time_phases=False)
    for h in HASHES:
        prove(h)
    ms = {h: [] for h in HASHES}
    for _ in range(reps):
        for h in HASHES:
            ms[h].append(wall_ms(pl, lambda: prove(h)))
    kk = {h: kernels(pl, lambda: prove(h)) for h in HASHES}                         # profiled in a run of its own
    for h in HASHES:
        res[h]["prove_wall_ms"] = stats(ms[h], 3)
        res[h]["prove_hash_kernels_us"] = round(sum(t for name, (c, t, b) in kk[h].items() if name.startswith(PREFIX[h] + "_")), 1)
        res[h]["prove_all_kernels_us"] = round(sum(t for c, t, b in kk[h].values()), 1)

    def ratio(key, a="blake3_256", b="blake2s"):
        return round(res[a][key]["median"] / res[b][key]["median"], 3)
    res["blake3_over_blake2s"] = {key: ratio(key) for key in res["blake3_256"] if isinstance(res["blake3_256"][key], dict)}
    res["reps"] = reps
    print(json.dumps(res, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
