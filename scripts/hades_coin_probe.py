#!/usr/bin/env python3
"""What the Poseidon public coin of the 252-bit field costs on one MI355X, written to profiles/hades_coin_probe.txt and quoted in
DESIGN.md 4.13c.  Kernel times are the library's own per-launch hipEvents on its stream (Planner.profile), warm, medians of --reps:
    chain    hades_coin_absorb in a reseed_elements of 2, 16 and 64 elements: microseconds per permutation (count / 2 + 2 of them)
    search   hades_coin_pow_grind over one full 2^20-nonce window (the fifth window of a search that finds nothing, isolated as the
             difference of two searches) against ms_poseidon252_permute on 2^20 states, same run
    draws    one hades_coin_draw of 1, 32 and 1024 elements (the last with its trailing hades_coin_advance)
    proof    pipeline.prove(hash="poseidon252", field=STARK252_FP) with coin=None (the SHA-256 byte coin) against coin="poseidon252", the
             fib AIR at 2^16 rows x 8 columns, blow-up 4, folding 8, 32 queries, 8 grinding bits: a host clock around the call, warm, the
             two alternating; and the transcript permutations of the algebraic proof, counted by the coin's rules
Nothing is asserted about the times.

    python scripts/hades_coin_probe.py [--log-t 16] [--log-window 20] [--reps 5] [--out profiles/hades_coin_probe.txt]
"""
import ctypes
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def random_elements(n, rng):
    """n canonical Montgomery elements as 4 n words: the top word below 2^58 < p / 2^192"""
    w = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2)
    w[:, 3] >>= np.uint64(6)
    return w.ravel()


def timed(pl, reps, labels, run):
    """median over `reps` warm rounds of the summed event time (us) of `labels` in one run()"""
    out = []
    for r in range(reps + 1):
        pl.profile(True)
        run()
        prof = pl.profile_read()
        if r:
            out.append(sum(prof[k]["total_us"] for k in labels if k in prof))
    pl.profile(False)
    return float(np.median(out)), out


def per_us(n, us):
    return n / us if us > 0 else float("nan")


def kernel_lines(pl, reps, lw=20):
    from ministark_amd import STARK252_FP as F, GpuVec
    from ministark_amd.coin import PoseidonCoin
    rng = np.random.default_rng(0xAD)
    coin = PoseidonCoin(pl, 3)
    lines = ["chain: hades_coin_absorb, one lane, one launch per reseed_elements (count / 2 + 1 hash_many permutations and the closing hash2)"]
    for count in (2, 16, 64):
        v = GpuVec.from_numpy(pl, random_elements(count, rng), F)
        perms = count // 2 + 2
        med, _ = timed(pl, reps, ["hades_coin_reseed_elements"], lambda: coin.reseed_elements(v))
        lines.append(f"  {count:3d} elements  {perms:3d} permutations  {med:10.1f} us  {med / perms:8.1f} us / permutation")
    lines.append("draws: one ms_hades_coin_draw (a lane per element; above 256 elements a trailing single-lane launch advances n_draws)")
    for count in (1, 32, 1024):
        med, _ = timed(pl, reps, ["hades_coin_draw"], lambda: coin.draw(F, count))
        lines.append(f"  {count:5d} elements  {med:10.1f} us")
    # the search: windows of 2^12, 2^14, 2^16, 2^18 nonces, then a full 2^20; 63 zero bits are not found
    short = sum(1 << k for k in range(12, lw, 2))            # lw: even, 14..24
    out = ctypes.c_uint64(0)
    grind = lambda most: pl.lib.ms_hades_coin_pow_grind(pl.handle, coin.ptr, 63, most, ctypes.byref(out))
    t_short, _ = timed(pl, reps, ["hades_coin_pow_grind"], lambda: grind(short))
    t_long, _ = timed(pl, reps, ["hades_coin_pow_grind"], lambda: grind(short + (1 << lw)))
    window = t_long - t_short
    states = GpuVec.from_numpy(pl, random_elements(3 << lw, rng), F)
    dst = GpuVec(pl, 3 << lw, F)
    permute = lambda: pl.lib.check(pl.lib.ms_poseidon252_permute(pl.handle, 1 << lw, states.ptr, dst.ptr))
    t_perm, _ = timed(pl, reps, ["poseidon252_permute"], permute)
    lines += [f"search: 2^{lw} permutations",
              f"  hades_coin_pow_grind, one 2^{lw}-nonce window  {window:10.1f} us  {per_us(1 << lw, window):8.2f} permutations / us   (the windows before it: {t_short:.1f} us)",
              f"  ms_poseidon252_permute, 2^{lw} states          {t_perm:10.1f} us  {per_us(1 << lw, t_perm):8.2f} permutations / us",
              f"  search / bulk permutation                    {per_us(window, t_perm):10.3f}"]
    return lines


def transcript_permutations(nchallenges, nood, nlayers, nrem, nqueries):
    """permutations of one proof without an extension trace, by the coin's rules: a reseed with a digest or an integer is one, a reseed
    with k elements k // 2 + 2, a draw of k elements k"""
    count = 1 + nchallenges                               # base root; composition coefficients
    count += 1 + 1                                        # composition root; z
    count += nood // 2 + 2 + nood + 2                     # OOD values; DEEP coefficients
    count += nlayers * 2                                  # per layer: root; alpha
    count += nrem // 2 + 2                                # remainder
    count += 1 + nqueries                                 # nonce; positions
    return count


def proof_lines(pl, log_t, reps):
    from ministark_amd import STARK252_FP as F, Matrix, pipeline
    from ministark_amd.api import F252_P, f252_to_mont_limbs
    n, blowup, folding, maxrem, bits, nq = 1 << log_t, 4, 8, 64, 8, 32
    cols, v = [[0] * n for _ in range(8)], [1, 2]
    for k in range(2, 8):
        v.append(v[k - 2] * v[k - 1] % F252_P)
    for r in range(n):
        for k in range(8):
            cols[k][r] = v[k]
        w = [v[6] * v[7] % F252_P]
        w.append(v[7] * w[0] % F252_P)
        for k in range(2, 8):
            w.append(w[k - 2] * w[k - 1] % F252_P)
        v = w
    trace = Matrix.from_numpy(pl, [np.concatenate([f252_to_mont_limbs(x) for x in c]).astype(np.uint64) for c in cols], F)
    comp, ce, nch = pipeline.fib_constraints(n, 8, F)
    hints = [cols[7][n - 1]]
    seed = bytes(range(31)) + b"\x01"                     # 32 bytes that both coins take: below p read little-endian
    ways = {"sha256 coin (coin=None)": None, "poseidon252 coin": "poseidon252"}
    times = {k: [] for k in ways}
    last = {}
    for r in range(reps + 1):                             # the first round warms plans, pools and kernels up
        for name, coin in ways.items():
            pl.sync()
            t = time.perf_counter()
            last[name] = pipeline.prove(pl, trace, comp, nch, hints, seed, blowup, folding, maxrem, bits, nq, hash="poseidon252", ce_blowup=ce, field=F, coin=coin)
            pl.sync()
            if r:
                times[name].append((time.perf_counter() - t) * 1e3)
    out = last["poseidon252 coin"]
    nrem = len(out["remainder_coeffs"]) // 4
    perms = transcript_permutations(nch, len(out["ood"][0]) + len(out["ood"][1]), len(out["fri_roots"]), nrem, nq)
    a, b = np.median(times["sha256 coin (coin=None)"]), np.median(times["poseidon252 coin"])
    lines = [f"proof: prove(hash=\"poseidon252\", field=STARK252_FP), fib AIR at 2^{log_t} rows x 8 columns, blow-up {blowup}, folding {folding}, {nq} queries, "
             f"{bits} grinding bits; host clock, warm, median of {reps}"]
    for name, t in times.items():
        lines.append(f"  {name:<26}{np.median(t):10.2f} ms   (all: {', '.join(f'{x:.2f}' for x in t)})")
    lines.append(f"  poseidon252 coin - sha256 coin {b - a:10.2f} ms")
    lines.append(f"  transcript permutations of the poseidon252-coin proof: {perms} ({len(out['fri_roots'])} FRI layers, {nrem} remainder coefficients), "
                 f"plus the search: nonce {out['nonce']}")
    return lines


def main():
    from ministark_amd import Planner
    pl = Planner(0)
    reps = int(arg("--reps", 5))
    lines = kernel_lines(pl, reps, int(arg("--log-window", 20))) + proof_lines(pl, int(arg("--log-t", 16)), reps)
    text = "\n".join(["scripts/hades_coin_probe.py: the Poseidon public coin of the 252-bit field on one MI355X (gfx950)"] + lines) + "\n"
    print(text, end="")
    with open(arg("--out", os.path.join(ROOT, "profiles", "hades_coin_probe.txt")), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
