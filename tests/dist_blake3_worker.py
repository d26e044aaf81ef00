"""Worker of tests/test_blake3_prover.py: python tests/dist_blake3_worker.py <rank> <world> <port> <outfile>.
Commits a column-sharded LDE with hash="blake3_256" over gloo on the simulator and writes one root (hex) per shape, then runs
distributed.prove_sharded(hash="blake3_256") on its columns; rank 0 compares every output with the single-device prove_phases."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch.distributed as dist  # noqa: E402

HASH = "blake3_256"
# (field, words per element, total columns, log2 trace rows, log2 blow-up): also read by the test.  The Fq3 shape's rows are 1 032 bytes:
# two chunks.
SHAPES = (("fp", 1, 5, 6, 2), ("fq3", 3, 43, 4, 2), ("fp", 1, 17, 5, 2))
# prove_sharded: log2 rows, columns, blow-up, folding, max remainder coefficients, grinding bits, queries
PROVE = (8, 8, 4, 8, 4, 6, 12)


def prove_inputs():
    """-> (columns, composition expression, ce_blowup, draws) of the sharded proof: the same on every rank and in the test"""
    import numpy as np
    from ministark_amd import pipeline
    log_rows, ncols, blowup, folding, max_rem, _, nq = PROVE
    n_t = 1 << log_rows
    rng = np.random.default_rng(300 + log_rows)
    cols = [rng.integers(0, (1 << 64) - (1 << 32) + 1, size=n_t, dtype=np.uint64) for _ in range(ncols)]
    comp, ce, nch = pipeline.fib_constraints(n_t, ncols)
    draws = pipeline.Draws(0xB3, ncols, nch, ce, nq, n_t * blowup, pipeline.fri_num_layers(n_t * blowup, blowup, folding, max_rem))
    return cols, comp, ce, draws


def main():
    rank, world, port, outfile = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import cref
    from tests import backends
    from tests.gloo_comm import GlooComm
    from ministark_amd import GOLDILOCKS_FP, GOLDILOCKS_FQ3
    from ministark_amd.distributed import lde_commit_sharded, owned_columns
    pl = backends.planner("emu")
    comm = GlooComm(pl)
    roots = []
    for name, V, total_cols, log_n, log_b in SHAPES:
        field = GOLDILOCKS_FQ3 if name == "fq3" else GOLDILOCKS_FP
        allc = [cref.random_elements((1 << log_n) * V, 3000 + c) for c in range(total_cols)]
        mine = [allc[c] for c in owned_columns(total_cols, rank, world)]
        root, _ = lde_commit_sharded(pl, comm, mine, total_cols, log_n, log_b, 7, field, hash=HASH)
        roots.append(root.hex())
    import numpy as np
    from ministark_amd import Matrix, pipeline
    from ministark_amd.distributed import prove_sharded
    log_rows, ncols, blowup, folding, max_rem, bits, _ = PROVE
    cols, comp, ce, draws = prove_inputs()
    got = prove_sharded(pl, comm, [cols[c] for c in owned_columns(ncols, rank, world)], ncols, log_rows, comp, draws, blowup, folding, max_rem, bits,
                        hash=HASH, ce_blowup=ce)
    ok = len(got["base_root"]) == 32
    if rank == 0:
        want = pipeline.prove_phases(pl, Matrix.from_numpy(pl, cols, GOLDILOCKS_FP), comp, draws, blowup, folding, max_rem, bits, hash=HASH, ce_blowup=ce)
        ok = (got["base_root"] == want["base_root"] and got["composition_root"] == want["composition_root"] and got["fri_roots"] == want["fri_roots"]
              and got["nonce"] == want["nonce"] and np.array_equal(got["remainder_coeffs"], want["remainder_coeffs"])
              and all(got["queries"][k] == getattr(want["queries"], k) for k in ("base_trace_proof", "composition_trace_proof"))
              and all(a["positions"] == b["positions"] and a["proof"] == b["proof"] for a, b in zip(got["fri_openings"], want["fri_openings"])))
    roots.append(f"prove:{'ok' if ok else 'MISMATCH'}:{got['base_root'].hex()}:{got['fri_roots'][-1].hex()}")
    with open(outfile, "w") as f:
        f.write("\n".join(roots))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
