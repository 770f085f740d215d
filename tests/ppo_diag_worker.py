"""One rank of the two-rank test of the PPO update diagnostics (tests/test_ppo_diag_gpu.py): a fresh process that joins the gloo group
from the environment (several ranks share the one GPU, DDRL_DIST_BACKEND=gloo), builds the Atari net through create_net and runs
PPO.learn on ITS shard of the batch the parent saved -- once with PPO_DIAGNOSTICS, once more from the same weights with the parent's
TARGET_KL -- and writes what it saw.

usage: python tests/ppo_diag_worker.py <outdir> <batch.npz> <bounds> <target_kl> <lr_scale>      e.g.  ... 0,40,64 0.0123 1.0
env:   RANK WORLD_SIZE MASTER_ADDR MASTER_PORT [LOCAL_RANK] [DDRL_DIST_BACKEND]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    outdir, batch_file, bounds = sys.argv[1], sys.argv[2], [int(t) for t in sys.argv[3].split(",")]
    target_kl, lr_scale = float(sys.argv[4]), float(sys.argv[5])
    import numpy as np
    import torch.distributed as dist

    from ddrl4nav_amd.dist import init_from_env
    import test_ppo_diag_gpu as T
    rank, world, _ = init_from_env()
    assert world == len(bounds) - 1
    batch = dict(np.load(batch_file))
    lo, hi = bounds[rank], bounds[rank + 1]
    diag_run = T.run_learn(batch, lo, hi, lr_scale=lr_scale, PPO_DIAGNOSTICS=True)
    stop_run = T.run_learn(batch, lo, hi, lr_scale=lr_scale, TARGET_KL=target_kl)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), diag=np.asarray(diag_run["diag"], np.float64),
             raw_sums=np.asarray(diag_run["raw_sums"], np.float64),
             params=diag_run["params"][-1], stop_yields=len(stop_run["items"]), stop_update_time=stop_run["update_time"],
             stop_params=stop_run["final_params"])
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
