#!/usr/bin/env python
"""Learning in place (config_nn.FRAMES_IN_PLACE: the conv1 kernels read the batch where it lies through a frame table; DESIGN.md section
6.3) against the staged paths, on one box, one fresh process per leg, the legs of a pass one after the other and the passes after one
another, so that the two paths of a comparison alternate.  A leg is  pool:work:path :

  pool   stacked (agent.DeviceRollout)  |  planes (agent.PlaneRollout)
  work   full_batch      one full-batch learn call of TRAINING_ITER_TIME = 10 iterations
         epoch_shuffled  one epoch of K shuffled minibatch steps
         epoch_in_order  the same epoch unshuffled
         kernels         one ddrl_ppo_iter / ddrl_ppo_iter_indexed of the whole batch under the per-kernel HIP events: ConvFwd1, ConvWgrad1
  path   staged (the knob off: the parent's path)  |  in_place (the knob on)

stacked:full_batch and stacked:epoch_in_order read contiguous frames either way and have no in_place leg.  Every run is one
PPO.learn call with the deferred read-back between a HIP-event pair (engine.Timer); a leg reports the median, the extremes and every
run.  Every leg runs in a process of its own under its own time limit; a leg that fails ends the tool: nothing more is started.
Prints one JSON line; --out appends every run of every leg to a text file.

    python tools/bench_in_place.py [--envs 256] [--steps 256] [--minibatches 4] [--runs 12] [--warmup 2] [--passes 2] [--legs ...] [--out F]
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

C, A = 4, 6
DEFAULT_LEGS = ("stacked:full_batch:staged", "planes:full_batch:staged", "planes:full_batch:in_place",
                "stacked:epoch_shuffled:staged", "stacked:epoch_shuffled:in_place", "planes:epoch_shuffled:staged",
                "planes:epoch_shuffled:in_place", "planes:epoch_in_order:staged", "planes:epoch_in_order:in_place",
                "planes:kernels:staged", "planes:kernels:in_place")
WORKS = ("full_batch", "epoch_shuffled", "epoch_in_order", "kernels")


def run_leg(pool, work, path, args):
    from ddrl4nav_amd.agent import DeviceRollout, PlaneRollout
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.data.frame_planes import planes_of
    from ddrl4nav_amd.engine import Timer
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.utils.recipe import make_weights
    N, T, K = args.envs, args.steps, args.minibatches
    B = N * T
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": C, "discrete_action": True,
           "discrete_actions": list(range(A)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg_nn = ConfigNN(env)
    iters = cfg_nn.TRAINING_ITER_TIME if work == "full_batch" else 1
    cfg_nn.TRAINING_ITER_TIME = iters
    cfg_nn.DEFERRED_LOSS_READBACK = True
    cfg_nn.FRAMES_IN_PLACE = path == "in_place"
    net = create_net({"config": BaseConfig(types.SimpleNamespace(task="bench_in_place", ip="127.0.0.1"), env), "config_nn": cfg_nn,
                      "config_env": env}, max_batch=B)
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
    for t in range(T + 1):
        ro.put_new_frames(t, frames[t], reset=True if t == 0 else resets[t])
        ro.act(t)
    for t in range(T + 1):
        ro.record(t, rewards[t], resets[min(t + 1, T)])
    ro.finish()
    data = ro.batch()
    del frames
    knobs = {"epoch_shuffled": (K, True, None, 1e-8), "epoch_in_order": (K, False, None, 1e-8), "full_batch": (1, False, None, 1e-8)}
    res = {"pool": pool, "work": work, "path": path, "device": torch.cuda.get_device_name(dev)}
    if work == "kernels":
        # one whole-batch iteration per run under the per-kernel events: the contiguous launch reads the materialised batch, the
        # indirect one the pool through the table of the same B samples
        hp, fp = net.hot_path, planes_of(data.states)
        f32 = lambda t: torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous()
        cols = [f32(data.actions), f32(data.old_logps), f32(data.advs), f32(data.values)[0].contiguous()]
        if path == "in_place":
            tab = fp.table(first=0, n=B)
            call = lambda: hp.ppo_iter_indexed(fp.pool, tab, *cols)
        else:
            batch = fp.stacks(0, B)
            call = lambda: hp.ppo_iter(batch, *cols)
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        hp.profile(True, acting=False)
        for _ in range(args.runs):
            call()
        torch.cuda.synchronize()
        prof = hp.profile_read()
        res["kernel_ms_per_call"] = {k: round(prof[k][0] / prof[k][1], 4) for k in ("ConvFwd1", "ConvWgrad1") if k in prof}
        res["calls"] = args.runs
        print(json.dumps(res))
        return
    timer, ms = Timer(), []
    for run in range(args.warmup + args.runs):
        net.load_state_dict(weights)          # every run starts from the same weights
        net.minibatch = knobs[work]
        torch.cuda.synchronize()
        timer.start()
        assert sum(1 for _ in net.learn(data)) == knobs[work][0] * iters
        timer.stop()
        torch.cuda.synchronize()
        if run >= args.warmup:
            ms.append(timer.elapsed_ms())
    # bytes held during learn: a fact of the tensors' sizes
    pool_t = {"frames": ro.frames} if pool == "stacked" else {"planes": ro.planes, "age": ro.age, "acting_scratch": ro._stack}
    held = {"plane_batch": net._plane_batch, "frame_table": net._frame_tab}
    if net._mb_stage is not None:
        held["minibatch_staging"], held["minibatch_table"] = net._mb_stage.frames, net._mb_stage.tab
    res.update({"runs_ms": [round(x, 3) for x in ms], "median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3),
                "max_ms": round(float(np.max(ms)), 3), "pool_bytes": {k: v.numel() * v.element_size() for k, v in pool_t.items()},
                "learner_frame_buffers_bytes": {k: v.numel() * v.element_size() for k, v in held.items() if v is not None}})
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--legs", default=",".join(DEFAULT_LEGS))
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds a leg's process may take")
    ap.add_argument("--out", default=None, help="append every run of every leg to this text file")
    ap.add_argument("--leg", default=None, help="run this one leg in this process (what the tool starts for every leg)")
    args = ap.parse_args()
    if args.leg is not None:
        pool, work, path = args.leg.split(":")
        assert pool in ("stacked", "planes") and work in WORKS and path in ("staged", "in_place"), args.leg
        return run_leg(pool, work, path, args)
    out = {"tool": "bench_in_place", "N": args.envs, "T": args.steps, "C": C, "K": args.minibatches, "runs": args.runs, "passes": []}
    for p_i in range(args.passes):
        legs = {}
        for name in args.legs.split(","):
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--envs", str(args.envs), "--steps",
                                    str(args.steps), "--minibatches", str(args.minibatches), "--runs", str(args.runs), "--warmup",
                                    str(args.warmup)], capture_output=True, text=True, timeout=args.leg_timeout, cwd=ROOT)
            except subprocess.TimeoutExpired:      # a leg that hung: nothing more is started on the GPU
                sys.exit("leg %s ran into its time limit of %d s" % (name, args.leg_timeout))
            if p.returncode != 0:      # a leg that failed: nothing more is started on the GPU
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit("leg %s failed with status %d" % (name, p.returncode))
            res = json.loads(p.stdout.strip().splitlines()[-1])
            out["device"] = res.pop("device")
            legs[name] = res
            if args.out:
                with open(args.out, "a") as f:
                    f.write("pass %d  %s  %s\n" % (p_i + 1, name, json.dumps(res)))
        cmp_ = {}
        for name, res in legs.items():      # in place against the staged path of the same pass, next to the staged leg's own spread
            pool, work, path = name.split(":")
            s = legs.get("%s:%s:staged" % (pool, work))
            if path == "in_place" and s and "median_ms" in res:
                cmp_["%s:%s" % (pool, work)] = {"in_place_minus_staged_ms": round(res["median_ms"] - s["median_ms"], 3),
                                                "staged_min_max_ms": [s["min_ms"], s["max_ms"]]}
        out["passes"].append({"legs": legs, "in_place_against_staged": cmp_})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
