"""One rank of the two-rank test of the running normalisation (tests/test_running_norm_gpu.py): a fresh process that joins the gloo
group from the environment (several ranks share the one GPU, DDRL_DIST_BACKEND=gloo), feeds ITS shard of the rows the parent saved to a
RunningNorm in two rounds -- each round several update() calls and one commit() -- and writes the state it ends with.

usage: python tests/running_norm_worker.py <outdir> <rows.npz> <bounds>      e.g.  ... 0,300,513
env:   RANK WORLD_SIZE MASTER_ADDR MASTER_PORT [LOCAL_RANK] [DDRL_DIST_BACKEND]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    outdir, rows_file, bounds = sys.argv[1], sys.argv[2], [int(t) for t in sys.argv[3].split(",")]
    import numpy as np
    import torch
    import torch.distributed as dist

    from ddrl4nav_amd.agent import RunningNorm
    from ddrl4nav_amd.dist import init_from_env
    rank, world, _ = init_from_env()
    assert world == len(bounds) - 1
    rows = np.load(rows_file)
    norm = RunningNorm((rows["round0"].shape[1],), "cuda")
    for r in range(2):
        x = torch.from_numpy(rows["round%d" % r][bounds[rank]:bounds[rank + 1]]).cuda()
        for part in torch.tensor_split(x, 3):      # several updates per commit: the pending sums accumulate
            if len(part):
                norm.update(part.contiguous())
        norm.commit()
    norm.freeze()
    torch.cuda.synchronize()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), state=norm.state.cpu().numpy(), affine=norm.affine.cpu().numpy())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
