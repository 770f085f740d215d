#!/usr/bin/env python
"""What the multi-robot navigation env costs (env/fleet_nav_env.py, csrc/fleetenv.hip), on one box in one
process, the legs alternating: ddrl_op_fleet_env_step at --rows rows (robots) as (n_worlds, R) = (rows, 1), (rows / 2, 2), (rows / 4, 4),
against two baselines -- ddrl_op_nav_env_step (env/device_nav_env.py) at N = rows, and a plain device-to-device copy of the same
rows * 31,508 observation bytes.  `calls` launches between one pair of device events give one sample (time per call); every leg is warmed
up first and reports the median, the p95 and the extremes of its samples.  The envs run under the same uniform-random actions, so robots
finish and respawn at the rate a fresh policy meets.  A second set of legs runs ddrl_op_fleet_env_step_final
against ddrl_op_fleet_env_step with the info word at R = 1, 2, 4, at the default max_steps and at max_steps = 1 (every robot that does
not collide truncates in every step), and the filing launch ddrl_op_file_flagged_rows of the terminal rows into pools of depth 1.  Prints
one JSON line.

    python tools/bench_device_fleet_env.py [--rows 512] [--calls 200] [--samples 30] [--warmup 2] [--ped-model walk] [--models]

--ped-model: the pedestrian model of every env above.  --models: instead of the legs above, ddrl_op_fleet_env_step
with the info word under "walk" and under "avoid" at R = 1, 2, 4, the six legs alternating.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_device_env import summary, timed  # noqa: E402
from tools.bench_device_nav_env import OBS_FLOATS, halves_spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512, help="robots in all: a multiple of 4")
    ap.add_argument("--calls", type=int, default=200, help="launches per sample")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ped-model", choices=("walk", "avoid"), default="walk")
    ap.add_argument("--models", action="store_true", help="only the walk / avoid comparison")
    args = ap.parse_args()
    if args.rows < 4 or args.rows % 4:
        sys.exit("--rows must be a positive multiple of 4")
    if not torch.cuda.is_available():
        sys.exit("bench_device_fleet_env needs a GPU: there is nothing to measure without one")
    from ddrl4nav_amd.env import DeviceNavEnv, FleetNavEnv
    rows = args.rows
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = torch.rand((rows, 2), device="cuda", generator=g) * torch.tensor([1.0, 2.0], device="cuda") - torch.tensor([0.0, 1.0], device="cuda")
    src = torch.rand((rows, OBS_FLOATS), device="cuda", generator=g)
    dst = torch.empty_like(src)
    if args.models:
        print(json.dumps({"tool": "bench_device_fleet_env", "rows": rows, "calls": args.calls, "device": torch.cuda.get_device_name(0),
                          "models": model_legs(args, actions)}))
        return
    envs = {"nav_env_step": DeviceNavEnv(rows, device="cuda", seed=1, ped_model=args.ped_model)}
    for R in (1, 2, 4):
        envs["fleet_env_step_R%d" % R] = FleetNavEnv(rows // R, R, device="cuda", seed=1, ped_model=args.ped_model)
    for env in envs.values():
        env.reset()

    def stepping(env):
        def run():
            for _ in range(args.calls):
                env.step(actions)
        return run

    def copies():
        for _ in range(args.calls):
            dst.copy_(src)

    legs = {k: stepping(env) for k, env in envs.items()}
    legs["d2d_copy"] = copies
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.samples):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    out = {"tool": "bench_device_fleet_env", "rows": rows, "calls": args.calls, "device": torch.cuda.get_device_name(0),
           "bytes_per_call": rows * OBS_FLOATS * 4}
    out.update({k: summary(v, per=args.calls) for k, v in ms.items()})
    for R in (1, 2, 4):
        k = "fleet_env_step_R%d" % R
        out[k]["worlds"] = rows // R
        out[k]["over_nav_env_step"] = round(out[k]["median_us"] / out["nav_env_step"]["median_us"], 3)
        out[k]["over_d2d_copy"] = round(out[k]["median_us"] / out["d2d_copy"]["median_us"], 3)
    out["final"] = final_legs(args, actions)
    print(json.dumps(out))


def model_legs(args, actions):
    """The step launch with the info word under both pedestrian models at R = 1, 2, 4, the six legs alternating."""
    from ddrl4nav_amd.env import FleetNavEnv
    rows = args.rows
    envs = {"%s_R%d" % (model, R): FleetNavEnv(rows // R, R, device="cuda", seed=1, emit_info=True, ped_model=model)
            for R in (1, 2, 4) for model in ("walk", "avoid")}
    for env in envs.values():
        env.reset()

    def stepping(env):
        def run():
            for _ in range(args.calls):
                env.step(actions)
        return run

    legs = {k: stepping(env) for k, env in envs.items()}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.samples):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    res = {k: summary(v, per=args.calls) for k, v in ms.items()}
    for R in (1, 2, 4):
        w, a = "walk_R%d" % R, "avoid_R%d" % R
        res[w]["spread_us"] = halves_spread(ms[w], per=args.calls)
        res[a]["over_walk"] = round(res[a]["median_us"] / res[w]["median_us"], 4)
        res[a]["minus_walk_us"] = round(res[a]["median_us"] - res[w]["median_us"], 3)
    return res


def final_legs(args, actions):
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.env import FleetNavEnv
    rows, out = args.rows, {}
    for name, max_steps in (("default_max_steps", 500), ("max_steps_1", 1)):
        envs = {}
        for R in (1, 2, 4):
            envs["fleet_env_step_info_R%d" % R] = FleetNavEnv(rows // R, R, device="cuda", seed=1, max_steps=max_steps, emit_info=True,
                                                               ped_model=args.ped_model)
            envs["fleet_env_step_final_R%d" % R] = FleetNavEnv(rows // R, R, device="cuda", seed=1, max_steps=max_steps, emit_final_obs=True,
                                                                ped_model=args.ped_model)
        for env in envs.values():
            env.reset()
        last = envs["fleet_env_step_final_R4"]
        pools = [torch.zeros((1,) + tuple(f.shape), device="cuda") for f in last.final_obs]
        count = torch.zeros(rows, dtype=torch.int32, device="cuda")
        slot = torch.zeros(rows, dtype=torch.int32, device="cuda")

        def stepping(env):
            def run():
                for _ in range(args.calls):
                    env.step(actions)
            return run

        def filing():                   # the info words and terminal rows the R = 4 env's last step left; an empty pool every time
            for _ in range(args.calls):
                count.zero_()
                ops.file_flagged_rows(last.info, list(zip(last.final_obs, pools)), count, slot)

        def zeroing():
            for _ in range(args.calls):
                count.zero_()

        legs = {k: stepping(env) for k, env in envs.items()}
        legs["file_flagged_rows_and_zero"], legs["zero_count"] = filing, zeroing
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(args.samples):
            for k, fn in legs.items():
                ms[k].append(timed(fn))
        res = {k: summary(v, per=args.calls) for k, v in ms.items()}
        for R in (1, 2, 4):
            a, b = "fleet_env_step_info_R%d" % R, "fleet_env_step_final_R%d" % R
            res[a]["spread_us"] = halves_spread(ms[a], per=args.calls)
            res[b]["minus_info_us"] = round(res[b]["median_us"] - res[a]["median_us"], 3)
            res[b]["same_state"] = bool(torch.equal(envs[a].state, envs[b].state))
        res["filing_us"] = round(res["file_flagged_rows_and_zero"]["median_us"] - res["zero_count"]["median_us"], 3)
        out[name] = res
    return out


if __name__ == "__main__":
    main()
