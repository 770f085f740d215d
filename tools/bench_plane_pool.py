#!/usr/bin/env python
"""The stacked experience pool (agent.DeviceRollout: every frame stored C times) against the single-frame pool (agent.PlaneRollout: stored
once, stacks assembled by csrc/fpool.hip where they are read), on one box, one fresh process per leg, one after
the other.  For each pool:

  acting          one rollout's acting phase, T + 1 steps of put_new_frames + act (the push kernel against copy + age + gather)
  epoch_shuffled  one epoch of K shuffled minibatch steps (ddrl_op_gather_minibatch against ddrl_op_gather_frame_stacks)
  epoch_in_order  the same epoch unshuffled (contiguous views against one gather per step into the staging buffer)
  full_batch      one full-batch learn call of TRAINING_ITER_TIME = 10 iterations (the plane pool materialises the batch first, once)

Every run is one acting phase or one PPO.learn call with the deferred read-back between a HIP-event pair (engine.Timer); a leg reports
the median, the extremes and every run, so the run-to-run spread stands next to the difference between the pools.  A leg that fails
ends the tool: nothing more is started.  Prints one JSON line.

    python tools/bench_plane_pool.py [--envs 256] [--steps 256] [--minibatches 4] [--runs 10] [--warmup 2] [--legs pool:leg,...]
"""
import argparse
import json
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOLS = ("stacked", "planes")
LEGS = ("acting", "epoch_shuffled", "epoch_in_order", "full_batch")
C, A = 4, 6


def run_leg(pool, leg, args):
    from ddrl4nav_amd.agent import DeviceRollout, PlaneRollout
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.engine import Timer
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.utils.recipe import make_weights
    N, T, K = args.envs, args.steps, args.minibatches
    B = N * T
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": C, "discrete_action": True,
           "discrete_actions": list(range(A)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg_nn = ConfigNN(env)
    iters = cfg_nn.TRAINING_ITER_TIME if leg == "full_batch" else 1      # a whole learn call at the default; ONE epoch of K steps
    cfg_nn.TRAINING_ITER_TIME = iters
    cfg_nn.DEFERRED_LOSS_READBACK = True
    net = create_net({"config": BaseConfig(types.SimpleNamespace(task="bench_plane_pool", ip="127.0.0.1"), env), "config_nn": cfg_nn,
                      "config_env": env}, max_batch=B if leg != "acting" else N)
    weights = {k: torch.from_numpy(v.copy()) for k, v in make_weights(0).items()}
    net.load_state_dict(weights)
    dev = net.device
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.empty((T + 1, N, 84, 84), dtype=torch.uint8, device=dev)
    for t in range(T + 1):      # in pieces: randint's int64 intermediate of the whole episode would be eight times the frames
        frames[t] = torch.randint(0, 256, frames[t].shape, dtype=torch.uint8, device=dev, generator=g)
    resets = (torch.rand((T + 1, N), device=dev, generator=g) < 0.01).to(torch.uint8)
    rewards = torch.randn((T + 1, N), device=dev, generator=g)
    ro = (DeviceRollout if pool == "stacked" else PlaneRollout)(net, N, horizon=T, channels=C, seed=1)

    def acting_phase():
        for t in range(T + 1):
            ro.put_new_frames(t, frames[t], reset=True if t == 0 else resets[t])
            ro.act(t)

    acting_phase()
    for t in range(T + 1):
        ro.record(t, rewards[t], resets[min(t + 1, T)])
    ro.finish()
    data = ro.batch()
    knobs = {"epoch_shuffled": (K, True, None, 1e-8), "epoch_in_order": (K, False, None, 1e-8), "full_batch": (1, False, None, 1e-8)}
    timer, ms = Timer(), []
    for run in range(args.warmup + args.runs):
        if leg != "acting":
            net.load_state_dict(weights)          # every run starts from the same weights
            net.minibatch = knobs[leg]
        torch.cuda.synchronize()
        timer.start()
        if leg == "acting":
            acting_phase()
        else:
            assert sum(1 for _ in net.learn(data)) == knobs[leg][0] * iters
        timer.stop()
        torch.cuda.synchronize()
        if run >= args.warmup:
            ms.append(timer.elapsed_ms())
    if pool == "stacked":
        pool_bytes = {"frames": ro.frames.numel()}
    else:
        pool_bytes = {"planes": ro.planes.numel(), "age": ro.age.numel(), "acting_scratch": ro._stack.numel()}
    held = {k: getattr(net, k) for k in ("_plane_batch",) if getattr(net, k, None) is not None}
    if net._mb_stage is not None:
        held["minibatch_staging"] = net._mb_stage.frames
    print(json.dumps({"pool": pool, "leg": leg, "device": torch.cuda.get_device_name(dev), "runs_ms": [round(x, 3) for x in ms],
                      "median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3),
                      "max_ms": round(float(np.max(ms)), 3), "pool_bytes": pool_bytes,
                      "learner_frame_buffers_bytes": {k: v.numel() for k, v in held.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default=",".join("%s:%s" % (p, l) for l in LEGS for p in POOLS))
    ap.add_argument("--leg", default=None, help="run this one leg in this process (what the tool starts for every leg)")
    args = ap.parse_args()
    if args.leg is not None:
        pool, leg = args.leg.split(":")
        assert pool in POOLS and leg in LEGS, args.leg
        return run_leg(pool, leg, args)
    out = {"tool": "bench_plane_pool", "N": args.envs, "T": args.steps, "C": C, "K": args.minibatches, "runs": args.runs, "legs": {}}
    for name in args.legs.split(","):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--envs", str(args.envs), "--steps", str(args.steps),
                            "--minibatches", str(args.minibatches), "--runs", str(args.runs), "--warmup", str(args.warmup)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        if p.returncode != 0:      # a leg that failed: nothing more is started on the GPU
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit("leg %s failed with status %d" % (name, p.returncode))
        res = json.loads(p.stdout.strip().splitlines()[-1])
        out["device"] = res.pop("device")
        out["legs"][name] = res
    legs = out["legs"]
    for leg in LEGS:      # planes against stacked, next to the stacked leg's own spread
        s, q = legs.get("stacked:" + leg), legs.get("planes:" + leg)
        if s and q:
            out.setdefault("planes_minus_stacked_ms", {})[leg] = round(q["median_ms"] - s["median_ms"], 3)
            out.setdefault("stacked_spread_ms", {})[leg] = round(s["max_ms"] - s["min_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
