#!/usr/bin/env python
"""Event times of DAgger's two new pieces next to what they sit beside, on BASELINE config 4's net
(NavPreNet1D x2 + GaussionActor(2)):

  (a) expert   ddrl_op_nav_expert (labels and the mixed action, one launch for all N envs) next to the env's own step launch at the
               same N: `calls` launches back to back per sample, per-launch time.
  (b) clone    one CloneTrainer.step on a minibatch of `batch` pool rows (gathers, the actor encoder's forward and backward, the MSE
               head, Adam over the arena) next to one PPO iteration of net.learn on a batch of the same size (both encoders, the PPO
               heads, Adam).

Every leg is warmed up first; a leg reports the median, the p95 and the extremes of its samples.  Prints one JSON line.

    python tools/bench_dagger.py [--envs 512] [--batch 1024] [--calls 100] [--samples 20] [--runs 10] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_device_env import summary, timed  # noqa: E402
from tools.bench_device_nav_env import make_net  # noqa: E402


def expert_legs(args):
    from ddrl4nav_amd.env import DeviceNavEnv, NavExpert
    N = args.envs
    env = DeviceNavEnv(N, device="cuda", seed=1)
    env.reset()
    expert = NavExpert(env)
    g = torch.Generator(device="cuda").manual_seed(0)
    policy = torch.rand((N, 2), device="cuda", generator=g)

    def mix():
        for k in range(args.calls):
            expert.mix(policy, 0.5, k)

    def step():
        for _ in range(args.calls):
            env.step(policy)

    legs = {"expert_mix": mix, "env_step": step}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.samples):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    out = {k: summary(v, per=args.calls) for k, v in ms.items()}
    out["expert_over_env_step"] = round(out["expert_mix"]["median_us"] / out["env_step"]["median_us"], 4)
    return out


def clone_legs(args):
    from ddrl4nav_amd.data import DemoPool, Experience
    from ddrl4nav_amd.env import DeviceNavEnv
    from ddrl4nav_amd.nn.dagger import CloneTrainer
    B = args.batch
    net = make_net(B, TRAINING_ITER_TIME=1)
    env = DeviceNavEnv(B, device=net.device, seed=1)
    obs = env.reset()
    g = torch.Generator(device=net.device).manual_seed(0)
    pool = DemoPool(env.state_shapes, 2, 2 * B, device=net.device, n_envs=B)
    pool.put(obs, torch.rand((B, 2), device=net.device, generator=g))
    trainer = CloneTrainer(net, pool, 1e-5)
    idx = torch.arange(B, dtype=torch.int32, device=net.device)
    rng = np.random.default_rng(0)
    data = Experience(states=[o.clone() for o in obs], advs=rng.normal(size=B).astype(np.float32),
                      actions=rng.uniform(0, 1, (B, 2)).astype(np.float32), old_logps=rng.normal(-1, 0.1, B).astype(np.float32),
                      values=rng.normal(size=(1, B)).astype(np.float32))

    def clone():
        trainer.step(idx, B)

    def ppo():
        for _ in net.learn(data):
            pass

    legs = {"clone_step": clone, "ppo_iteration": ppo}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.runs):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    out = {k: summary(v, unit="ms") for k, v in ms.items()}
    out["clone_over_ppo"] = round(out["clone_step"]["median_ms"] / out["ppo_iteration"]["median_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dagger needs a GPU")
    out = {"tool": "bench_dagger", "device": torch.cuda.get_device_name(0), "N": args.envs, "batch": args.batch,
           "expert": expert_legs(args), "clone": clone_legs(args)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
