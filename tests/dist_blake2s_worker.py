"""Worker of tests/test_blake2s_sharded.py: python tests/dist_blake2s_worker.py <rank> <world> <port> <outfile>.
Commits a column-sharded LDE with hash="blake2s" over gloo on the simulator and writes one root (hex) per shape."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch.distributed as dist  # noqa: E402

# (field, words per element, total columns, log2 trace rows, log2 blow-up): also read by the test
SHAPES = (("fp", 1, 5, 6, 2), ("fq3", 3, 3, 5, 3), ("fp", 1, 8, 7, 2))


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
        root, _ = lde_commit_sharded(pl, comm, mine, total_cols, log_n, log_b, 7, field, hash="blake2s")
        roots.append(root.hex())
    with open(outfile, "w") as f:
        f.write("\n".join(roots))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
