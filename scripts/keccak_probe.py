#!/usr/bin/env python3
"""Keccak-256 and SHA3-256 commitments next to SHA-256 and BLAKE2s-256 on one GPU, on the same buffers in the same run, after a
warm-up, timed with the library's per-launch hipEvents on its stream (ms_profile_*) and, for whole calls, a host clock around work
that ends in a device synchronise:
    (a) leaves of 8 and of 32 Fp columns x 2^22 rows             Matrix.hash_rows
    (b) a 2^22-leaf tree                                         MerkleTree(leaves)      (level launches + subtrees + top); the
        merge-level rate is that of the level launches, reported as the time of a level of 2^21 parents
    (c) prove_phases at configs[4]'s shape (2^22 rows x 8 columns, blow-up 4, folding 8), one proof per hash
Each case alternates the hashes, `--reps` times, and reports the median, and the ratio of every figure to SHA-256's.

    python scripts/keccak_probe.py [--reps 5] [--json out.json] [--no-prove]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ministark_amd import GL_P, DeviceBytes, Matrix, MerkleTree, Planner, pipeline  # noqa: E402

HASHES = ("sha256", "blake2s", "keccak256", "sha3_256")
PREFIX = {"sha256": "sha256", "blake2s": "blake2s", "keccak256": "keccak", "sha3_256": "keccak"}      # of the profiled kernel names


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


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    pl = Planner(0)
    rng = np.random.default_rng(5)
    res = {h: {} for h in HASHES}

    # (a) leaves
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
            res[h][f"leaves_{ncols}x2^22_us"] = round(float(np.median(us[h])), 1)
        del m

    # (b) a 2^22-leaf tree: total and the merge-level rate
    leaves = DeviceBytes(pl, n * 32)
    raw = rng.integers(0, 256, size=n * 32, dtype=np.uint8)
    pl.lib.check(pl.lib.ms_upload(pl.handle, leaves.ptr, raw.ctypes.data, n * 32))
    for h in HASHES:
        MerkleTree(pl, leaves, n, h)
    per = {h: {"tree_us": [], "tree_wall_ms": [], "level_2^21_parents_us": [], "top_us": []} for h in HASHES}
    for _ in range(reps):
        for h in HASHES:
            k = kernels(pl, lambda: MerkleTree(pl, leaves, n, h))
            per[h]["tree_us"].append(sum(t for c, t, b in k.values()))
            lvl = k[f"{PREFIX[h]}_merkle_level"]
            per[h]["level_2^21_parents_us"].append(lvl[1] / (lvl[2] / 96.0) * (1 << 21))
            per[h]["top_us"].append(k[f"{PREFIX[h]}_merkle_top"][1])
            per[h]["tree_wall_ms"].append(wall_ms(pl, lambda: MerkleTree(pl, leaves, n, h)))
    for h in HASHES:
        for key, v in per[h].items():
            res[h][f"tree_2^22_{key}"] = round(float(np.median(v)), 3 if key.endswith("ms") else 1)
    del leaves

    # (c) prove_phases at configs[4]'s shape
    if "--no-prove" not in sys.argv:
        log_t, blowup, folding, ncols = 22, 4, 8, 8
        n_t = 1 << log_t
        cols = [rng.integers(0, GL_P, size=n_t, dtype=np.uint64) for _ in range(ncols)]
        trace = Matrix.from_numpy(pl, cols)
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
        kk = {h: kernels(pl, lambda: prove(h)) for h in HASHES}
        for h in HASHES:
            res[h]["prove_ms"] = round(float(np.median(ms[h])), 3)
            res[h]["prove_ms_all"] = [round(x, 3) for x in ms[h]]
            res[h]["prove_hash_kernels_us"] = round(sum(t for name, (c, t, b) in kk[h].items() if name.startswith(PREFIX[h] + "_")), 1)
            res[h]["prove_all_kernels_us"] = round(sum(t for c, t, b in kk[h].values()), 1)
    res["ratio_to_sha256"] = {h: {k: round(v / res["sha256"][k], 3) for k, v in res[h].items() if not isinstance(v, list) and res["sha256"].get(k)}
                              for h in HASHES if h != "sha256"}
    res["reps"] = reps
    print(json.dumps(res, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
