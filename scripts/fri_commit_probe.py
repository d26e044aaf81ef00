"""The FRI commit phase with and without the device-resident public coin, at configs[4]'s shape (2^22 x 8 trace, blow-up 4, folding 8:
a first layer of 2^24 evaluations), on one MI355X.  Warm, median of REPS runs, wall clock between two stream synchronisations (phase
(i) contains host waits by construction, so the host clock is the one that sees all of it):
  (i)   the phase as pipeline.prove_phases runs it: per layer commit, download the root, fold with a host alpha; then the remainder's
        inverse transform
  (ii)  the phase as pipeline.prove runs it: per layer commit, reseed with the root on the device, draw alpha into device memory, fold
        from there; the remainder, reseed with its coefficients; roots and alphas downloaded once at the end
  (iii) the coin's launches alone, us per reseed_digest + draw and per reseed_elements of 20 and 64 elements (a chain of 2 compressions
        per element on one lane after the parallel element digests)
    python scripts/fri_commit_probe.py > profiles/fri_commit_probe.txt"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from ministark_amd import GOLDILOCKS_FP as FP, GpuVec, Matrix, MerkleTree, Planner, Radix2EvaluationDomain, apply_drp, pipeline  # noqa: E402
from ministark_amd.coin import PublicCoin  # noqa: E402

LOG_N, BLOWUP, FOLDING, MAXREM = int(os.environ.get("LOG_LDE", "24")), 4, 8, 64
REPS = int(os.environ.get("REPS", "11"))
P = (1 << 64) - (1 << 32) + 1


def remainder(cur, n):
    rem = Matrix([cur.clone()]).bit_reverse_rows().into_polynomials(Radix2EvaluationDomain(n, 1, FP)).columns[0]
    return rem, max(n // BLOWUP, 1)


def phase_host(pl, layer0, alphas, hash):
    cur, n, roots = layer0, len(layer0), []
    for a in alphas:
        roots.append(MerkleTree.from_fri_layer(cur, FOLDING, hash).root())
        cur = apply_drp(cur, a, FOLDING, 1)
        n //= FOLDING
    rem, k = remainder(cur, n)
    return roots, rem.to_numpy()[:k]


def phase_coin(pl, layer0, nlayers, hash, coin):
    cur, n, trees, alphas = layer0, len(layer0), [], []
    for _ in range(nlayers):
        tree = MerkleTree.from_fri_layer(cur, FOLDING, hash)
        coin.reseed_digest(tree.root_ptr())
        alphas.append(coin.draw(FP, 1))
        trees.append(tree)
        cur = apply_drp(cur, alphas[-1], FOLDING, 1)
        n //= FOLDING
    rem, k = remainder(cur, n)
    coin.reseed_elements(GpuVec(pl, k, FP, ptr=rem.ptr))
    return [t.root() for t in trees], [a.to_numpy() for a in alphas], rem.to_numpy()[:k]


def median_ms(pl, fn):
    times = []
    for _ in range(REPS + 2):
        pl.sync()
        t = time.perf_counter()
        fn()
        pl.sync()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times[2:]), min(times[2:])


def main():
    pl = Planner(0)
    n = 1 << LOG_N
    layer0 = GpuVec.from_numpy(pl, np.random.default_rng(1).integers(0, P, size=n, dtype=np.uint64))
    nlayers = pipeline.fri_num_layers(n, BLOWUP, FOLDING, MAXREM)
    alphas = [np.array([a], dtype=np.uint64) for a in np.random.default_rng(2).integers(0, P, size=nlayers, dtype=np.uint64)]
    print(f"first layer 2^{LOG_N}, folding {FOLDING}, {nlayers} layers, median (min) of {REPS} warm runs")
    for hash in ("sha256", "blake2s"):
        coin = PublicCoin(pl, bytes(32), pipeline.pow_hash(hash))
        host = median_ms(pl, lambda: phase_host(pl, layer0, alphas, hash))
        dev = median_ms(pl, lambda: phase_coin(pl, layer0, nlayers, hash, coin))
        print(f"{hash:8s} (i) host alphas, root download per layer: {host[0]:.3f} ms ({host[1]:.3f})   (ii) device coin: {dev[0]:.3f} ms ({dev[1]:.3f})")
        digest, elems = GpuVec.from_numpy(pl, np.arange(4, dtype=np.uint64)), GpuVec.from_numpy(pl, np.arange(64, dtype=np.uint64))

        def pair():
            for _ in range(100):
                coin.reseed_digest(digest.ptr)
                coin.draw(FP, 1)
        print(f"{hash:8s} (iii) reseed_digest + draw: {median_ms(pl, pair)[0] * 10:.2f} us per pair (100 pairs back to back)")
        for count in (20, 64):
            view = GpuVec(pl, count, FP, ptr=elems.ptr)

            def many():
                for _ in range(20):
                    coin.reseed_elements(view)
            us = median_ms(pl, many)[0] * 1e3 / 20
            print(f"{hash:8s} (iii) reseed_elements({count}): {us:.2f} us per call, {us / count:.3f} us per element")


if __name__ == "__main__":
    main()
