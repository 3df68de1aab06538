"""worker of tests/test_gpu_update.py::test_pool_sharded_update_matches_the_unsharded_solve: two PROCESSES share GPU 0 (gloo for
the host side, the one-shot exchange for the device's, no RCCL -- it refuses two ranks on one device), each holding half of every
bucket.  After a first solve, a block of swaps is applied with every rank updating its own slice in local positions
(cfmm.problem.shard_updates) -- rank 1's slices untouched, so it calls with count = 0 -- and one pool on rank 0 grows to hold the
network's largest reserve (the reproducible mode's exponent must be re-reduced over the ranks).  Rank 0 writes the ranks' solves
and the unsharded fresh solve of the same network to argv[1]."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cfmm-routing-code_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

import cfmm  # noqa: E402
from cfmm import synthetic  # noqa: E402
from cfmm.problem import shard_range, shard_updates  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    net = synthetic.config("C3", scale=0.1, seed=4)
    n = net["n_tokens"]
    after, changes = synthetic.swap_block(net, 0.02, seed=5)
    # keep only the entries of rank 0's slices: rank 1 has nothing to update in any bucket
    block = {}
    for key, (pos, R) in changes.items():
        m = len(net[key]["Ra"]) if isinstance(key, str) else net["gn"][key]["R"].shape[1]
        lo, hi = shard_range(m, 0, world)
        sel = (pos >= lo) & (pos < hi)
        block[key] = (pos[sel], R[:, sel].copy())
    pos, R = block["cp2"]                                   # one pool on rank 0 grows past every reserve of the network
    top = max([max(net[k]["Ra"].max(), net[k]["Rb"].max()) for k in ("cp2", "w2")] + [b["R"].max() for b in net["gn"].values()])
    R[:, 0] *= 4.0 * top / R[:, 0].max()
    netB = synthetic.copy_network(net)
    for key, (pos, R) in block.items():
        if isinstance(key, str):
            netB[key]["Ra"][pos] = R[0]; netB[key]["Rb"][pos] = R[1]
        else:
            netB["gn"][key]["R"][:, pos] = R
    nu0 = net["c"] * np.exp(np.random.default_rng(3).normal(0, 0.02, n))
    p = cfmm.distributed.sharded_problem(synthetic.copy_network(net), cfmm.Arbitrage(net["c"]), dist=dist, device=0, allreduce="oneshot", rccl=False)
    p.ctx.set_deterministic(True)
    p.solve(tol=1e-6, method="lbfgs")
    counts = {}
    for key, (pos, R) in block.items():
        m = len(net[key]["Ra"]) if isinstance(key, str) else net["gn"][key]["R"].shape[1]
        lp, lR, _ = shard_updates(m, rank, world, pos, R)
        counts[str(key)] = int(len(lp))
        p.update_bucket(key, lp, lR)
    v = p.solve(nu0=nu0, tol=1e-6, method="lbfgs")
    mine = dict(value=v, status=p.status, evals=p.stats["evals"], nu=p.nu.tolist(), counts=counts)
    box = [None] * world
    dist.all_gather_object(box, mine)
    ref = None
    if rank == 0:                                           # the unsharded fresh upload of the new network, same GPU, after the ranks
        q = cfmm.Problem.from_network(netB, utility=cfmm.Arbitrage(net["c"]), deterministic=True)
        ref = dict(value=q.solve(nu0=nu0, tol=1e-6, method="lbfgs"), evals=q.stats["evals"], nu=q.nu.tolist(), status=q.status)
        q.close()
    p.close()
    dist.barrier()
    if rank == 0:
        with open(sys.argv[1], "w") as fh:
            json.dump(dict(world=world, ranks=box, unsharded=ref), fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
