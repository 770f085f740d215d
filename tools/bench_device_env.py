#!/usr/bin/env python
"""What a device env costs (env/device_env.py, csrc/denv.hip), on one box in one process, the legs of each
measurement alternating:

  (a) kernel   ddrl_op_env_step for N envs against a plain device-to-device copy of the same N * 7056 bytes -- what a rollout spends
               to take a ready-made device frame, so the yardstick.  `calls` launches between one pair of device events give one
               sample (time per call); the samples of the two legs alternate.
  (b) acting   one rollout's acting phase on a PlaneRollout, T steps between one pair of events: act -> env.step rendering into the pool
               row -> record -> put_new_frames, against the same phase fed pre-made device frames, rewards and dones (act -> record ->
               put_new_frames with its copy).

Every leg is warmed up first; a leg reports the median, the p95 and the extremes of its samples.  Prints one JSON line.

    python tools/bench_device_env.py [--game pong] [--envs 256] [--steps 256] [--calls 200] [--samples 30] [--runs 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, A = 4, 6


def summary(ms, per=1.0, unit="us"):
    x = np.asarray(ms, np.float64) * (1000.0 if unit == "us" else 1.0) / per
    return {"median_" + unit: round(float(np.median(x)), 3), "p95_" + unit: round(float(np.percentile(x, 95)), 3),
            "min_" + unit: round(float(x.min()), 3), "max_" + unit: round(float(x.max()), 3), "samples": len(x)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_legs(args):
    from ddrl4nav_amd.env import DeviceEnv
    N = args.envs
    env = DeviceEnv(args.game, N, device="cuda", seed=1)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = torch.randint(0, A, (N,), device="cuda", generator=g).to(torch.float32)
    src = torch.randint(0, 256, (N, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    dst = torch.empty_like(src)

    def steps():
        for _ in range(args.calls):
            env.step(actions)

    def copies():
        for _ in range(args.calls):
            dst.copy_(src)

    for _ in range(args.warmup):
        steps()
        copies()
    torch.cuda.synchronize()
    ms = {"env_step": [], "d2d_copy": []}
    for _ in range(args.samples):
        ms["env_step"].append(timed(steps))
        ms["d2d_copy"].append(timed(copies))
    out = {k: summary(v, per=args.calls) for k, v in ms.items()}
    out["bytes_per_call"] = N * 7056
    out["step_over_copy"] = round(out["env_step"]["median_us"] / out["d2d_copy"]["median_us"], 3)
    return out


def acting_legs(args):
    from ddrl4nav_amd.agent import PlaneRollout
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.env import DeviceEnv
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.utils.recipe import make_weights
    N, T = args.envs, args.steps
    cfg_env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": C, "discrete_action": True,
               "discrete_actions": list(range(A)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    net = create_net({"config": BaseConfig(types.SimpleNamespace(task="bench_device_env", ip="127.0.0.1"), cfg_env),
                      "config_nn": ConfigNN(cfg_env), "config_env": cfg_env}, max_batch=N)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_weights(0).items()})
    env = DeviceEnv(args.game, N, device="cuda", seed=1)
    ro = PlaneRollout(net, N, horizon=T, channels=C, seed=1)
    # the pre-made leg replays frames, rewards and dones that the env itself produced (recorded once, outside the timed window)
    frames = torch.empty((T + 1, N, 84, 84), dtype=torch.uint8, device="cuda")
    rewards = torch.empty((T, N), dtype=torch.float32, device="cuda")
    dones = torch.empty((T, N), dtype=torch.uint8, device="cuda")
    env.reset(frame_out=frames[0])
    ro.put_new_frames(0, frames[0], reset=True)
    for t in range(T):
        _, r, d = env.step(ro.act(t), frame_out=frames[t + 1])
        rewards[t].copy_(r)
        dones[t].copy_(d)
        ro.record(t, r, d)
        ro.put_new_frames(t + 1, frames[t + 1])

    def with_env():
        for t in range(T):
            frame, r, d = env.step(ro.act(t), frame_out=ro.new_frame_row(t + 1))
            ro.record(t, r, d)
            ro.put_new_frames(t + 1, frame)

    def premade():
        for t in range(T):
            ro.act(t)
            ro.record(t, rewards[t], dones[t])
            ro.put_new_frames(t + 1, frames[t + 1])

    for _ in range(args.warmup):
        with_env()
        premade()
    torch.cuda.synchronize()
    ms = {"device_env": [], "premade_frames": []}
    for _ in range(args.runs):
        ms["device_env"].append(timed(with_env))
        ms["premade_frames"].append(timed(premade))
    out = {k: summary(v, unit="ms") for k, v in ms.items()}
    out["device_env_over_premade"] = round(out["device_env"]["median_ms"] / out["premade_frames"]["median_ms"], 4)
    out["env_steps_per_s_device_env"] = round(N * T / (out["device_env"]["median_ms"] / 1000.0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", choices=("pong", "catch"), default="pong")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--calls", type=int, default=200, help="launches per sample of the kernel legs")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--runs", type=int, default=10, help="timed acting phases per leg")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_device_env needs a GPU: there is nothing to measure without one")
    out = {"tool": "bench_device_env", "game": args.game, "N": args.envs, "T": args.steps, "device": torch.cuda.get_device_name(0),
           "kernel": kernel_legs(args), "acting": acting_legs(args)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
