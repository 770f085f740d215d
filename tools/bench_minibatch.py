#!/usr/bin/env python
"""What PPO minibatch epochs cost on the Atari fast path (nn/minibatch.py): one epoch of K minibatch steps with the
shuffle's staging gather, the same epoch on contiguous views, and one full-batch iteration of the parent path -- on one net and one
batch, interleaved A B C A B C, the median over the runs; every run is one PPO.learn call with the deferred read-back (one
synchronisation) between a HIP-event pair (engine.Timer).  Prints one JSON line.

    python tools/bench_minibatch.py [--batch 65536] [--minibatches 4] [--runs 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.engine import Timer
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.utils.recipe import make_weights
    B, K, C, A = args.batch, args.minibatches, 4, 6
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": C, "discrete_action": True,
           "discrete_actions": list(range(A)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg_nn = ConfigNN(env)
    cfg_nn.TRAINING_ITER_TIME = 1
    cfg_nn.DEFERRED_LOSS_READBACK = True
    net = create_net({"config": BaseConfig(types.SimpleNamespace(task="bench_minibatch", ip="127.0.0.1"), env), "config_nn": cfg_nn,
                      "config_env": env}, max_batch=B)
    weights = {k: torch.from_numpy(v.copy()) for k, v in make_weights(0).items()}
    dev = net.device
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.empty((B, C, 84, 84), dtype=torch.uint8, device=dev)
    for lo in range(0, B, 4096):      # in pieces: randint's int64 intermediate of the whole batch would be eight times the frames
        frames[lo:lo + 4096] = torch.randint(0, 256, frames[lo:lo + 4096].shape, dtype=torch.uint8, device=dev, generator=g)
    rnd = lambda: torch.randn(B, device=dev, generator=g)
    data = types.SimpleNamespace(states=[frames], actions=torch.randint(0, A, (B,), device=dev, generator=g).float(),
                                 old_logps=-float(np.log(A)) + 0.3 * rnd(), advs=rnd(), values=rnd().view(1, B))
    variants = {"epoch_shuffled": (K, True, None, 1e-8), "epoch_in_order": (K, False, None, 1e-8), "full_batch_iteration": (1, False, None, 1e-8)}
    timer, ms = Timer(), {k: [] for k in variants}
    for run in range(args.warmup + args.runs):
        for name, knobs in variants.items():      # interleaved: every variant sees the same drift of clocks and temperature
            net.load_state_dict(weights)          # every run starts from the same weights (Adam's moments run on: same arithmetic cost)
            net.minibatch = knobs
            torch.cuda.synchronize()
            timer.start()
            n = sum(1 for _ in net.learn(data))
            timer.stop()
            torch.cuda.synchronize()
            assert n == knobs[0]
            if run >= args.warmup:
                ms[name].append(timer.elapsed_ms())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    row_bytes = C * 84 * 84
    out = {"tool": "bench_minibatch", "device": torch.cuda.get_device_name(dev), "B": B, "K": K, "C": C, "runs": args.runs,
           "median_ms": {k: round(v, 3) for k, v in med.items()},
           "min_ms": {k: round(float(np.min(v)), 3) for k, v in ms.items()},
           "max_ms": {k: round(float(np.max(v)), 3) for k, v in ms.items()},
           "gather_bytes_per_epoch": 2 * B * (row_bytes + 16),
           "shuffle_cost_ms": round(med["epoch_shuffled"] - med["epoch_in_order"], 3),
           "gather_gbps_if_all_of_it": round(2 * B * (row_bytes + 16) / max(med["epoch_shuffled"] - med["epoch_in_order"], 1e-9) / 1e6, 1),
           "epoch_over_full_batch": round(med["epoch_in_order"] / med["full_batch_iteration"], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
