#!/usr/bin/env python3
"""Poseidon commitments over the 252-bit field next to SHA-256 and Keccak-256 on one GPU, on the same buffers, after a warm-up, timed
with the library's per-launch hipEvents on its stream (ms_profile_*) and, for whole calls, a host clock around work that ends in a
device synchronise.  Steps, each in a child process of its own under its own time limit (the driver stops at the first that fails):
    static   no GPU: the gfx950 assembly of ms_poseidon.cpp -- VGPRs, scratch and vector instructions of every kernel, and the static
             count per permutation: 8 full rounds of the whole loop body and 83 partial rounds of the body without what the uniform
             branches on `full` skip (the divergent conditional-subtraction blocks counted as taken)
    merge    the merge level at 2^20 parents                     the level launches of a 2^21-leaf tree less those of a 2^20-leaf one
    leaves   leaves of 8 and of 32 Fp252 columns x 2^20 rows     Matrix.hash_rows
    tree     a whole 2^20-leaf tree, its top split out           MerkleTree(leaves)
    permute  ms_poseidon252_permute at 2^20 states
    prove    prove_phases, fib AIR, 2^16 rows x 8 columns over the 252-bit field, blow-up 4, folding 8, one proof per hash
    counters the vector instructions the hardware counts (SQ_INSTS_VALU, a run of its own under rocprofv3 --pmc) in one launch each of
             the permutation kernel, the sponge (8 columns) and the merge level at 2^20 lanes: per permutation, next to the static count
For the Poseidon kernels the fraction of the VALU issue peak is (static instructions per permutation x permutations / 64) / time over
bench_objects.VALU_ISSUE_PEAK = 1024 SIMDs x 2.4 GHz / 4 wave instructions a second.

    python scripts/poseidon_probe.py [--reps 5] [--out profiles/poseidon_probe.txt] [--steps static,merge,...]
"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

HASHES = ("sha256", "keccak256", "poseidon252")
PREFIX = {"sha256": "sha256", "keccak256": "keccak", "poseidon252": "poseidon252"}      # of the profiled kernel names
STEPS = {"static": 600, "merge": 240, "leaves": 240, "tree": 240, "permute": 120, "prove": 420, "counters": 300}       # seconds
N = 1 << 20


# ---- static: the assembly ---------------------------------------------------------------------------------------------------------------

def _loop_counts(body):
    """body: the lines of one kernel, labels with the compiler's loop comments included -> (VALU in the round loop, VALU the uniform
    forward branches in it skip).  The round loop is the innermost one the compiler annotates; its blocks are the labels it marks
    `in Loop: Header=<that label>`."""
    labels = {m.group(1): i for i, line in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", line)] if m}
    head = [m.group(1) for line in body for m in [re.match(r"^\.L(BB\d+_\d+):.*This Inner Loop Header", line)] if m]
    if not head:
        return None
    members = [i for i, line in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", line) and (f"Header={head[0]} " in line or line.startswith(f".L{head[0]}:"))]
    start = min(members)
    after = [i for i in labels.values() if i > max(members)]
    end = min(after) if after else len(body)
    valu = [1 if re.match(r"^v_", line) else 0 for line in body]
    skipped = 0
    for i in range(start, end):
        m = re.match(r"^s_cbranch_(vcc|scc)\w+\s+(\.LBB\d+_\d+)", body[i])
        if m and i < labels[m.group(2)] < end:
            skipped += sum(valu[i:labels[m.group(2)]])
    return sum(valu[start:end]), skipped


def step_static():
    import isa_count
    from ministark_amd import build as msbuild
    src = os.path.join(msbuild.CSRC, "ms_poseidon.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "ms_poseidon.s")
        flags = [f for f in msbuild.FLAGS if f not in ("-shared", "-fPIC")]
        subprocess.run([msbuild.HIPCC] + flags + ["-S", "--cuda-device-only", src, "-o", out], check=True, stderr=subprocess.DEVNULL)
        meta = isa_count.meta(out)
        res = {}
        name, body = None, []
        for line in list(open(out)) + ["end:\n"]:
            s = line.strip()
            m = re.match(r"^(_Z\w+):", s)
            if m or s == "end:":
                if name and "poseidon252" in name:
                    short = re.search(r"poseidon252_[a-z_]+?(?=E[A-Z]|$)", name).group(0)
                    ins = [x if x.startswith(".LBB") else x.split(";")[0].strip() for x in body if x and not x.startswith((";", "//"))]
                    md = meta.get(name, {})
                    loop = _loop_counts(ins)
                    res[short] = {"valu_static": sum(1 for x in ins if x.startswith("v_")), "vgpr": md.get("vgpr_count"), "sgpr": md.get("sgpr_count"),
                                  "scratch_bytes": md.get("private_segment_fixed_size"), "vgpr_spills": md.get("vgpr_spill_count")}
                    if loop:
                        full, skipped = loop
                        res[short].update({"valu_full_round": full, "valu_partial_round": full - skipped,
                                           "valu_per_permutation": 8 * full + 83 * (full - skipped)})
                name, body = (m.group(1) if m else None), []
                continue
            if s.startswith(".end_amdhsa_kernel") or s.startswith(".Lfunc_end"):
                continue
            if name and not s.startswith(".") or re.match(r"^\.LBB\d+_\d+:", s):
                body.append(s)
    return res


# ---- the device steps -------------------------------------------------------------------------------------------------------------------

def _setup():
    import numpy as np
    from ministark_amd import Planner
    return Planner(0), np.random.default_rng(5), np


def _elements(np, rng, n):
    """n canonical Fp252 elements as words: any value below 2^251 < p"""
    w = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2)
    w[:, 3] &= np.uint64((1 << 59) - 1)
    return w.ravel()


def _kernels(pl, fn):
    pl.sync()
    pl.profile(True)
    fn()
    pl.sync()
    prof = pl.profile_read()
    pl.profile(False)
    return {k: (v["calls"], v["total_us"], v["bytes_per_call"] * v["calls"]) for k, v in prof.items()}


def _wall_ms(pl, fn):
    pl.sync()
    t = time.perf_counter()
    fn()
    pl.sync()
    return (time.perf_counter() - t) * 1e3


def _median(np, v, digits=1):
    return round(float(np.median(v)), digits)


def _leaf_buffer(pl, np, rng, n):
    from ministark_amd import DeviceBytes
    leaves = DeviceBytes(pl, n * 32)
    raw = _elements(np, rng, n)                                  # canonical elements: valid Poseidon digests, and bytes like any for the others
    pl.lib.check(pl.lib.ms_upload(pl.handle, leaves.ptr, raw.ctypes.data, n * 32))
    return leaves


def step_merge(reps):
    """the level of 2^20 parents alone: the level launches of a 2^21-leaf tree less those of a 2^20-leaf tree over the same buffer -- the
    smaller tree's launches are the larger one's without its first.  (Averaging over all level launches would charge the big level
    with the small ones, which cost one permutation's latency however few nodes they have.)"""
    from ministark_amd import MerkleTree
    pl, rng, np = _setup()
    leaves = _leaf_buffer(pl, np, rng, 2 * N)
    for h in HASHES:
        MerkleTree(pl, leaves, 2 * N, h)
    us = {h: [] for h in HASHES}
    for _ in range(reps):
        for h in HASHES:
            level = [_kernels(pl, lambda: MerkleTree(pl, leaves, n, h))[f"{PREFIX[h]}_merkle_level"] for n in (2 * N, N)]
            assert level[0][0] == level[1][0] + 1                # one launch more
            us[h].append(level[0][1] - level[1][1])
    return {h: {"level_2^20_parents_us": _median(np, us[h])} for h in HASHES}


def step_leaves(reps):
    from ministark_amd import STARK252_FP, Matrix
    pl, rng, np = _setup()
    res = {h: {} for h in HASHES}
    for ncols in (8, 32):
        m = Matrix.from_numpy(pl, [_elements(np, rng, N) for _ in range(ncols)], STARK252_FP)
        for h in HASHES:
            m.hash_rows(h)
        us = {h: [] for h in HASHES}
        for _ in range(reps):
            for h in HASHES:
                k = _kernels(pl, lambda: m.hash_rows(h))
                us[h].append(sum(t for name, (c, t, b) in k.items() if name.endswith("_rows")))
        for h in HASHES:
            res[h][f"leaves_{ncols}x2^20_us"] = _median(np, us[h])
        del m
    return res


def step_tree(reps):
    from ministark_amd import MerkleTree
    pl, rng, np = _setup()
    leaves = _leaf_buffer(pl, np, rng, N)
    for h in HASHES:
        MerkleTree(pl, leaves, N, h)
    per = {h: {"tree_us": [], "top_us": [], "tree_wall_ms": []} for h in HASHES}
    for _ in range(reps):
        for h in HASHES:
            k = _kernels(pl, lambda: MerkleTree(pl, leaves, N, h))
            per[h]["tree_us"].append(sum(t for c, t, b in k.values()))
            per[h]["top_us"].append(k[f"{PREFIX[h]}_merkle_top"][1])       # Poseidon: the one launch of the levels of <= 256 parents
            per[h]["tree_wall_ms"].append(_wall_ms(pl, lambda: MerkleTree(pl, leaves, N, h)))
    return {h: {f"tree_2^20_{key}": _median(np, v, 3 if key.endswith("ms") else 1) for key, v in per[h].items()} for h in HASHES}


def step_permute(reps):
    from ministark_amd import STARK252_FP, GpuVec, poseidon252_permute
    pl, rng, np = _setup()
    states = GpuVec.from_numpy(pl, _elements(np, rng, 3 * N), STARK252_FP)
    poseidon252_permute(pl, states)
    us = []
    for _ in range(reps):
        us.append(_kernels(pl, lambda: poseidon252_permute(pl, states))["poseidon252_permute"][1])
    return {"poseidon252": {"permute_2^20_states_us": _median(np, us), "permute_ns_per_state": round(float(np.median(us)) * 1e3 / N, 2)}}


def step_prove(reps):
    from ministark_amd import STARK252_FP, Matrix, pipeline
    from ministark_amd.api import F252_P, f252_to_mont_limbs
    pl, rng, np = _setup()
    n, ncols, blowup, folding = 1 << 16, 8, 4, 8
    v = [1, 2]
    for k in range(2, 8):
        v.append(v[k - 2] * v[k - 1] % F252_P)
    cols = [[0] * n for _ in range(ncols)]
    for r in range(n):                                           # the fib AIR's trace
        for k in range(8):
            cols[k][r] = v[k]
        w = [v[6] * v[7] % F252_P]
        w.append(v[7] * w[0] % F252_P)
        for k in range(2, 8):
            w.append(w[k - 2] * w[k - 1] % F252_P)
        v = w
    trace = Matrix.from_numpy(pl, [np.concatenate([f252_to_mont_limbs(x) for x in c]).astype(np.uint64) for c in cols], STARK252_FP)
    comp, ce, nch = pipeline.fib_constraints(n, ncols, STARK252_FP)
    nlayers = pipeline.fri_num_layers(n * blowup, blowup, folding, 64)
    draws = pipeline.Draws(7, ncols, nch, ce, 32, n * blowup, nlayers, modulus=F252_P)
    draws.hints = [cols[7][n - 1]]

    def prove(h):
        return pipeline.prove_phases(pl, trace, comp, draws, blowup, folding, 64, 8, hash=h, ce_blowup=ce, time_phases=False, field=STARK252_FP)
    for h in HASHES:
        prove(h)
    ms = {h: [] for h in HASHES}
    for _ in range(reps):
        for h in HASHES:
            ms[h].append(_wall_ms(pl, lambda: prove(h)))
    kk = {h: _kernels(pl, lambda: prove(h)) for h in HASHES}
    return {h: {"prove_2^16_ms": _median(np, ms[h], 3), "prove_2^16_ms_all": [round(x, 3) for x in ms[h]],
                "prove_hash_kernels_us": round(sum(t for name, (c, t, b) in kk[h].items() if name.startswith(PREFIX[h] + "_")), 1),
                "prove_all_kernels_us": round(sum(t for c, t, b in kk[h].values()), 1)} for h in HASHES}


def step_pmc_child(reps):
    """under rocprofv3: one launch each of the three kernels at 2^20 lanes (the tree's first level is its widest launch)"""
    from ministark_amd import STARK252_FP, GpuVec, Matrix, MerkleTree, poseidon252_permute
    pl, rng, np = _setup()
    poseidon252_permute(pl, GpuVec.from_numpy(pl, _elements(np, rng, 3 * N), STARK252_FP))
    Matrix.from_numpy(pl, [_elements(np, rng, N) for _ in range(8)], STARK252_FP).hash_rows("poseidon252")
    MerkleTree(pl, _leaf_buffer(pl, np, rng, 2 * N), 2 * N, "poseidon252")
    pl.sync()
    return {}


def step_counters(reps):
    import csv
    import glob
    import shutil
    if shutil.which("rocprofv3") is None:
        return {"counters": "not measured: no rocprofv3"}
    names = ("SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_BUSY_CYCLES", "GRBM_GUI_ACTIVE")
    with tempfile.TemporaryDirectory() as out:
        cmd = ["rocprofv3", "--kernel-trace", "--pmc", *names, "-d", out, "-o", "t", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--step", "pmc_child"]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS["counters"] - 20)
        hits = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
        if run.returncode != 0 or not hits:
            return {"counters": f"not measured: rocprofv3 exit status {run.returncode}"}
        rows = list(csv.DictReader(open(hits[0])))
    perms = {"poseidon252_permute": 1, "poseidon252_rows": 5, "poseidon252_merge_level": 1}      # permutations a lane
    res = {}
    for kernel, per_lane in perms.items():
        mine = [r for r in rows if kernel in r["Kernel_Name"] and int(float(r["Grid_Size"])) == N]
        ids = sorted({r["Dispatch_Id"] for r in mine})
        if len(ids) != 1:
            res[kernel] = f"not measured: {len(ids)} launches of 2^20 lanes"
            continue
        c = {r["Counter_Name"]: float(r["Counter_Value"]) for r in mine}
        res[kernel] = {"counters": c, "valu_per_permutation_counted": round(c["SQ_INSTS_VALU"] * 64.0 / (N * per_lane), 1)}
    return {"counters": res}


# ---- the driver -------------------------------------------------------------------------------------------------------------------------

def _merge(into, part):
    for k, v in part.items():
        if isinstance(v, dict):
            _merge(into.setdefault(k, {}), v)
        else:
            into[k] = v


def _derive(res):
    """ratios to SHA-256, and the Poseidon kernels' fraction of the VALU issue peak from the static counts"""
    from bench_objects import VALU_ISSUE_PEAK                    # 1024 SIMDs x 2.4 GHz / 4 wave instructions a second
    sha = res.get("sha256", {})
    res["ratio_to_sha256"] = {h: {k: round(v / sha[k], 3) for k, v in res.get(h, {}).items() if not isinstance(v, list) and sha.get(k)}
                              for h in HASHES if h != "sha256"}
    st, pos = res.get("static", {}), res.get("poseidon252", {})
    frac = {}
    for kernel, key, perms in (("poseidon252_permute", "permute_2^20_states_us", N), ("poseidon252_merge_level", "level_2^20_parents_us", N),
                               ("poseidon252_rows", "leaves_8x2^20_us", 5 * N), ("poseidon252_rows", "leaves_32x2^20_us", 17 * N)):
        per = st.get(kernel, {}).get("valu_per_permutation")
        if per and pos.get(key):
            frac[key] = round(per * perms / 64.0 / (pos[key] * 1e-6) / VALU_ISSUE_PEAK, 4)
    res["poseidon252_frac_of_valu_issue_peak"] = frac
    counted = {}                                                 # the same fraction from the instructions the hardware counted
    cnt = res.get("counters", {})
    for kernel, key, perms in (("poseidon252_permute", "permute_2^20_states_us", N), ("poseidon252_merge_level", "level_2^20_parents_us", N),
                               ("poseidon252_rows", "leaves_8x2^20_us", 5 * N)):
        per = cnt.get(kernel, {}).get("valu_per_permutation_counted") if isinstance(cnt, dict) and isinstance(cnt.get(kernel), dict) else None
        if per and pos.get(key):
            counted[key] = round(per * perms / 64.0 / (pos[key] * 1e-6) / VALU_ISSUE_PEAK, 4)
    res["poseidon252_frac_of_valu_issue_peak_counted"] = counted


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    if "--step" in sys.argv:                                     # a child: one step, one JSON line
        step = sys.argv[sys.argv.index("--step") + 1]
        fn = globals()["step_" + step]
        print("RESULT " + json.dumps(fn() if step == "static" else fn(reps)))
        return 0
    steps = sys.argv[sys.argv.index("--steps") + 1].split(",") if "--steps" in sys.argv else list(STEPS)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res, status = {"reps": reps}, 0
    for step in steps:
        try:                                                     # a fresh process per step, under the step's own limit
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(reps)], capture_output=True,
                                 text=True, timeout=STEPS[step])
        except subprocess.TimeoutExpired:
            res["stopped_at"], status = f"{step}: time limit of {STEPS[step]} s", 124
            break
        line = [x for x in run.stdout.splitlines() if x.startswith("RESULT ")]
        if run.returncode != 0 or not line:
            res["stopped_at"], status = f"{step}: exit status {run.returncode}: {run.stderr[-400:]}", run.returncode or 1
            break                                                # nothing more is started on the device after a failure
        _merge(res, {"static": json.loads(line[0][7:])} if step == "static" else json.loads(line[0][7:]))
        print(f"[poseidon_probe] {step} done", file=sys.stderr, flush=True)
    _derive(res)
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
