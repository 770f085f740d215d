"""One rank of the two-rank test of the PPO minibatch epochs (tests/test_minibatch_gpu.py): a fresh process that joins the gloo group
from the environment (several ranks share the one GPU, DDRL_DIST_BACKEND=gloo), builds the Atari net with K = 2, shuffling and
"batch" advantage normalisation, runs PPO.learn on ITS shard of the batch the parent saved and writes what it saw.

usage: python tests/minibatch_worker.py <outdir> <batch.npz> <bounds>      e.g.  ... 0,20,37
env:   RANK WORLD_SIZE MASTER_ADDR MASTER_PORT [LOCAL_RANK] [DDRL_DIST_BACKEND]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    outdir, batch_file, bounds = sys.argv[1], sys.argv[2], [int(t) for t in sys.argv[3].split(",")]
    import numpy as np
    import torch.distributed as dist

    from ddrl4nav_amd.dist import init_from_env
    from ddrl4nav_amd.nn import minibatch as M
    import minibatch_ref as R
    rank, world, _ = init_from_env()
    assert world == len(bounds) - 1
    batch = dict(np.load(batch_file))
    lo, hi = bounds[rank], bounds[rank + 1]
    _, weights = R.batch_of(R.cell(bounds[-1]))          # the recipe weights of the parent's cell
    K = 2
    net = R.make_net(weights, bounds[1] - bounds[0], PPO_MINIBATCHES=K, PPO_SHUFFLE=True, NORMALIZE_ADVANTAGE="batch")
    items = R.run_learn(net, batch, lo, hi)
    first_lo, first_hi = M.split(hi - lo, K)[0]
    first = M.epoch_order(net._seed + rank, 0, 0, hi - lo)[first_lo:first_hi].numpy()
    state = R.state_of(net)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), params=state["params"], m=state["m"], v=state["v"], step=state["step"],
             yields=len(items), affine=net._mb_stage.affine.cpu().numpy(), first=first,
             losses=np.asarray([[ld[k] for k in ("ActorLoss", "VLoss", "EntLoss")] for ld, _ in items], np.float64))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
