"""One rank of a multi-process RCCL run that takes summaries (tests/test_gpu_summary_ranks.py).

    RANK=r WORLD_SIZE=W MASTER_ADDR=127.0.0.1 MASTER_PORT=p \
        python tests/helpers/summary_worker.py OUTDIR N TOPOLOGY ALGORITHM SEED ROUNDS

Like rccl_worker.py: joins a gloo group (used once, for rank 0's RCCL id), creates its slab on
device GP_BENCH_DEVICE, steps ROUNDS rounds, then takes the GLOBAL summary (collective), the LOCAL
one, and the GLOBAL one again, and writes their bytes with its slab's range to OUTDIR/rank<r>.npz.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(argv):
    out, n, topo, alg, seed, rounds = argv[1], int(argv[2]), argv[3], argv[4], int(argv[5]), int(argv[6])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    device = int(os.environ.get("GP_BENCH_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gossipprotocol_amd import Simulation
    from tests.summary_ref import raw
    sim = Simulation(n, topo, alg, seed=seed, device=device, rank=rank, world=world, dist=dist)
    alerts = sim.step(rounds)
    g1 = raw(sim.summary(1e-10, "global"))
    loc = raw(sim.summary(1e-10, "local"))
    g2 = raw(sim.summary(1e-10, "global"))
    more = sim.step(3)  # the run goes on after the summaries
    info = sim.info()
    np.savez(os.path.join(out, f"rank{rank}.npz"), alerts=np.asarray(alerts + more, np.int64),
             first=np.int64(info.slab_first), count=np.int64(info.slab_count),
             g1=np.frombuffer(g1, np.uint8), g2=np.frombuffer(g2, np.uint8), loc=np.frombuffer(loc, np.uint8))
    sim.close()
    dist.barrier()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
