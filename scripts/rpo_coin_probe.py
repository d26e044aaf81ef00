#!/usr/bin/env python3
"""What the RPO-256 public coin costs on one MI355X, written to profiles/rpo_coin_probe.txt and quoted in DESIGN.md 4.13b:
    chain    time per permutation of a 64-permutation draw, lane-per-element (shipped) against the one-lane form of the same kernel
    search   permutations per second of rpo_coin_pow_grind over a 2^24 window against rpo256_merge_level on 2^24 nodes, same run
             (both from scripts/rpo_coin_probe.hip: hipEvents, resident data, warm; built here when the binary is missing)
    proof    pipeline.prove(hash="rpo256", coin="rpo256") against pipeline.prove(hash="rpo256") (the SHA-256 coin, the prover as it was)
             at 2^22 rows x 8 columns, blow-up 4, folding 8, 32 queries, 8 grinding bits: a host clock around the call (it ends in the
             download of the openings), warm, the two alternating; and the transcript permutations of the algebraic proof, counted
Nothing is asserted about the times.

    python scripts/rpo_coin_probe.py [--log-t 22] [--reps 5] [--out profiles/rpo_coin_probe.txt] [--build-only]
"""
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
SRC, BIN = os.path.join(HERE, "rpo_coin_probe.hip"), os.path.join(HERE, "rpo_coin_probe_bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def build():
    deps = [SRC] + [os.path.join(ROOT, "ministark_amd", "csrc", f) for f in ("rpo_coin_kernels.h", "rpo_kernels.h", "gl.h", "gl_dev.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function", SRC, "-o", BIN])
    return BIN


def transcript_permutations(nchallenges, nood, nlayers, nrem, nqueries):
    """permutations of one Fp proof without an extension trace, by the coin's rules: create; per reseed one, per block of absorbed
    elements one; a draw of k words from a freshly reseeded coin refills (k - 1) // 8 times"""
    refills = lambda k: (k - 1) // 8
    count = 1                                             # create
    count += 1 + refills(nchallenges)                     # base root; composition coefficients
    count += 1 + refills(1)                               # composition root; z
    count += nood // 8 + 1 + refills(nood + 2)            # OOD values; DEEP coefficients
    count += nlayers * (1 + refills(1))                   # per layer: root; alpha
    count += nrem // 8 + 1                                # remainder
    count += 1 + refills(nqueries)                        # nonce; positions
    return count


def proof_times(log_t, reps):
    from ministark_amd import GL_P, GOLDILOCKS_FP as FP, Matrix, Planner, pipeline
    pl = Planner(0)
    n, blowup, folding, maxrem, bits, nq = 1 << log_t, 4, 8, 64, 8, 32
    rng = np.random.default_rng(0xC5)
    trace = Matrix.from_numpy(pl, [rng.integers(0, GL_P, size=n, dtype=np.uint64) for _ in range(8)], FP)
    comp, ce, nch = pipeline.fib_constraints(n)
    seed = bytes(range(32))
    ways = {"sha256 coin (coin=None)": None, "rpo256 coin": "rpo256"}
    times = {k: [] for k in ways}
    last = {}
    for r in range(reps + 1):                             # the first round warms plans, pools and kernels up
        for name, coin in ways.items():
            pl.sync()
            t = time.perf_counter()
            last[name] = pipeline.prove(pl, trace, comp, nch, [5], seed, blowup, folding, maxrem, bits, nq, hash="rpo256", ce_blowup=ce, coin=coin)
            pl.sync()
            if r:
                times[name].append((time.perf_counter() - t) * 1e3)
    out = last["rpo256 coin"]
    perms = transcript_permutations(nch, len(out["ood"][0]) + len(out["ood"][1]), len(out["fri_roots"]), len(out["remainder_coeffs"]), nq)
    lines = [f"proof: prove(hash=\"rpo256\") at 2^{log_t} rows x 8 columns, blow-up {blowup}, folding {folding}, {nq} queries, {bits} grinding bits; host clock, warm, median of {reps}"]
    for name, v in times.items():
        lines.append(f"  {name:<26}{np.median(v):10.2f} ms   (all: {', '.join(f'{x:.2f}' for x in v)})")
    lines.append(f"  rpo256 coin - sha256 coin {np.median(times['rpo256 coin']) - np.median(times['sha256 coin (coin=None)']):10.2f} ms")
    lines.append(f"  transcript permutations of the rpo256-coin proof: {perms} ({len(out['fri_roots'])} FRI layers, {len(out['remainder_coeffs'])} remainder coefficients), "
                 f"plus the search: nonce {out['nonce']}")
    return lines


def main():
    exe = build()
    if "--build-only" in sys.argv:
        return
    kernels = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    if kernels.returncode != 0 or "FAILED" in kernels.stdout:
        raise SystemExit("rpo_coin_probe_bin failed:\n" + kernels.stdout + kernels.stderr)
    lines = kernels.stdout.rstrip().splitlines() + proof_times(int(arg("--log-t", 22)), int(arg("--reps", 5)))
    text = "\n".join(["scripts/rpo_coin_probe.py: the RPO-256 public coin on one MI355X (gfx950)"] + lines) + "\n"
    print(text, end="")
    with open(arg("--out", os.path.join(ROOT, "profiles", "rpo_coin_probe.txt")), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
