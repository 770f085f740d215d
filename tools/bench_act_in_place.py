#!/usr/bin/env python
"""Acting in place (config_nn.ACT_IN_PLACE: PlaneRollout.act reads its slot of the single-frame pool through a frame table, one
ddrl_op_frame_slot launch + ddrl_forward_indexed) against the gathered path and the stacked pool, on one box, one
fresh process per leg, the legs of a pass one after the other and the passes after one another, so that the legs alternate.  Legs:

  stacked    agent.DeviceRollout: put_new_frames (the push kernel) + act on the stacked slot
  gathered   agent.PlaneRollout, the knob off (the parent's path): copy + age + gather into the scratch + act
  in_place   agent.PlaneRollout, the knob on: copy + slot launch + act through the table
  kernels    a contiguous and an indirect forward of `envs` samples under the per-kernel HIP events (ddrl_profile_enable(on = 1)): the
             ActConvs time of each

A run of the first three is one rollout's acting phase, T + 1 steps of put_new_frames + act, between a HIP-event pair (engine.Timer); a
leg reports the median, the extremes and every run.  Every leg runs in a process of its own under its own time limit; a leg that fails
ends the tool: nothing more is started.  The yardstick of the in-place leg is the gathered leg of the same pass: the tool reports
in-place minus gathered next to the gathered leg's own min - max, and calls the in-place leg faster only where its median lies below the
gathered leg's minimum in every pass.  Prints one JSON line; --out appends every run of every leg to a text file.

    python tools/bench_act_in_place.py [--envs 256] [--steps 256] [--runs 12] [--warmup 2] [--passes 2] [--legs ...] [--out F]
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
LEGS = ("stacked", "gathered", "in_place", "kernels")


def run_leg(leg, args):
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.agent import DeviceRollout, PlaneRollout
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.engine import Timer
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.utils.recipe import make_weights
    N, T = args.envs, args.steps
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": C, "discrete_action": True,
           "discrete_actions": list(range(A)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg_nn = ConfigNN(env)
    cfg_nn.ACT_IN_PLACE = leg == "in_place"
    net = create_net({"config": BaseConfig(types.SimpleNamespace(task="bench_act_in_place", ip="127.0.0.1"), env), "config_nn": cfg_nn,
                      "config_env": env}, max_batch=N)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_weights(0).items()})
    dev = net.device
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.empty((T + 1, N, 84, 84), dtype=torch.uint8, device=dev)
    for t in range(T + 1):      # in pieces: randint's int64 intermediate of the whole episode would be eight times the frames
        frames[t] = torch.randint(0, 256, frames[t].shape, dtype=torch.uint8, device=dev, generator=g)
    resets = (torch.rand((T + 1, N), device=dev, generator=g) < 0.01).to(torch.uint8)
    res = {"leg": leg, "device": torch.cuda.get_device_name(dev)}
    if leg == "kernels":
        # slot T of a filled plane pool, once as the gathered stacks and once through its table: the same bytes
        hp = net.hot_path
        ro = PlaneRollout(net, N, horizon=T, channels=C, seed=1, act_in_place=False)
        for t in range(T + 1):
            ro.put_new_frames(t, frames[t], reset=True if t == 0 else resets[t])
        stacks = ro.stacks(T)
        tab = ops.frame_table_planes(ro.planes, ro.age, C, torch.empty((N, 4), dtype=torch.int32, device=dev), first=T * N, n=N)
        calls = {"contiguous": lambda: hp.forward(stacks, seed=1, stream_id=T),
                 "indirect": lambda: hp.forward_indexed(ro.planes, tab, N, seed=1, stream_id=T)}
        res["ActConvs_us_per_call"] = {}
        for name, call in calls.items():
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            hp.profile(True, acting=True)
            for _ in range(args.runs):
                call()
            torch.cuda.synchronize()
            ms, n_calls = hp.profile_read()["ActConvs"]
            hp.profile(False)
            assert n_calls == args.runs
            res["ActConvs_us_per_call"][name] = round(1000.0 * ms / n_calls, 2)
        res["calls"] = args.runs
        print(json.dumps(res))
        return
    ro = (DeviceRollout if leg == "stacked" else PlaneRollout)(net, N, horizon=T, channels=C, seed=1)
    assert leg == "stacked" or ro.act_in_place is (leg == "in_place")
    timer, ms = Timer(), []
    for run in range(args.warmup + args.runs):
        torch.cuda.synchronize()
        timer.start()
        for t in range(T + 1):
            ro.put_new_frames(t, frames[t], reset=True if t == 0 else resets[t])
            ro.act(t)
        timer.stop()
        torch.cuda.synchronize()
        if run >= args.warmup:
            ms.append(timer.elapsed_ms())
    # bytes held while acting: a fact of the tensors' sizes
    if leg == "stacked":
        held = {"frames": ro.frames}
    else:
        held = {"planes": ro.planes, "age": ro.age, "acting_scratch": ro._stack, "slot_table": ro._slot_tab}
    res.update({"runs_ms": [round(x, 3) for x in ms], "median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3),
                "max_ms": round(float(np.max(ms)), 3),
                "pool_bytes": {k: v.numel() * v.element_size() for k, v in held.items() if v is not None}})
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--leg-timeout", type=int, default=180, help="seconds a leg's process may take")
    ap.add_argument("--out", default=None, help="append every run of every leg to this text file")
    ap.add_argument("--leg", default=None, help="run this one leg in this process (what the tool starts for every leg)")
    args = ap.parse_args()
    if args.leg is not None:
        assert args.leg in LEGS, args.leg
        return run_leg(args.leg, args)
    out = {"tool": "bench_act_in_place", "N": args.envs, "T": args.steps, "C": C, "runs": args.runs, "passes": []}
    for p_i in range(args.passes):
        legs = {}
        for name in args.legs.split(","):
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--envs", str(args.envs), "--steps",
                                    str(args.steps), "--runs", str(args.runs), "--warmup", str(args.warmup)], capture_output=True,
                                   text=True, timeout=args.leg_timeout, cwd=ROOT)
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
        gathered, in_place, stacked = legs.get("gathered"), legs.get("in_place"), legs.get("stacked")
        if gathered and in_place:      # in place against the gathered leg of the same pass, next to the gathered leg's own spread
            cmp_ = {"in_place_minus_gathered_ms": round(in_place["median_ms"] - gathered["median_ms"], 3),
                    "gathered_min_max_ms": [gathered["min_ms"], gathered["max_ms"]],
                    "in_place_below_gathered_min": in_place["median_ms"] < gathered["min_ms"]}
            if stacked:                # reported next to it; not a gate
                cmp_["in_place_minus_stacked_ms"] = round(in_place["median_ms"] - stacked["median_ms"], 3)
                cmp_["gathered_minus_stacked_ms"] = round(gathered["median_ms"] - stacked["median_ms"], 3)
        out["passes"].append({"legs": legs, "in_place_against_gathered": cmp_})
    verdicts = [p["in_place_against_gathered"].get("in_place_below_gathered_min") for p in out["passes"]]
    if verdicts and all(v is not None for v in verdicts):
        out["in_place_faster_in_every_pass"] = all(verdicts)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
