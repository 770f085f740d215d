#!/usr/bin/env python3
"""Measurement of the running observation / return normalisation (csrc/runnorm.hip) at the BASELINE config-4
shapes: 512 envs whose observation components are 960 (laser), 5 (goal vector) and 6,912 (pedestrian map) floats per step, and the
131,072 returns of a 256-step rollout.  Not the headline bench (bench.py is); needs a GPU; prints one JSON line.

  ops      device-event time per call of the five operators, the median of REPEATS windows of CALLS back-to-back calls each (a call
           is 1 - 2 launches of a few microseconds: single calls would time the event pair), with the bytes each call has to move
  acting   StateRollout's acting phase at 512 envs (puts from device tensors + act per step, bootstrap, finish) with the knobs on and
           off, the two rollouts interleaved in one process, median of REPEATS rounds

Usage: python tools/bench_running_norm.py [T] [repeats]      (T: steps of the acting measurement, default 32)"""
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddrl4nav_amd import ops  # noqa: E402

N_ENVS, T_FULL = 512, 256
COMPONENTS = (("laser", (1, 960)), ("vector", (5,)), ("ped_map", (3, 48, 48)))
CALLS = 50


def window_ms(fn, calls=CALLS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def timed(fn, repeats):
    window_ms(fn, 5)  # warm-up: code objects, the allocator
    times = sorted(window_ms(fn) for _ in range(repeats))
    return {"us_per_call": round(statistics.median(times) * 1e3, 2), "min_us": round(times[0] * 1e3, 2), "max_us": round(times[-1] * 1e3, 2)}


def bench_ops(repeats):
    g = torch.Generator(device="cuda").manual_seed(6)
    out = {}
    shapes = [(name, N_ENVS, int(torch.Size(shape).numel())) for name, shape in COMPONENTS] + [("returns", N_ENVS * T_FULL, 1)]
    for name, n, d in shapes:
        x = torch.randn((n, d), device="cuda", generator=g)
        y = torch.empty_like(x)
        sums = torch.zeros(1 + 2 * d, dtype=torch.float64, device="cuda")
        ws = torch.empty(ops.column_moments_ws_floats(n, d), dtype=torch.float32, device="cuda")
        state = ops.running_state(d, "cuda")
        affine = ops.running_affine(state, 1e-8)
        row = {"n": n, "d": d, "bytes_read": n * d * 4}
        row["column_moments"] = timed(lambda: ops.column_moments(x, d, sums=sums, ws=ws), repeats)
        row["running_merge"] = timed(lambda: ops.running_merge(sums, state), repeats)
        row["running_affine"] = timed(lambda: ops.running_affine(state, 1e-8, affine=affine), repeats)
        row["normalize_columns"] = timed(lambda: ops.normalize_columns(x, affine, 10.0, out=y), repeats)
        row["normalize_in_place"] = timed(lambda: ops.normalize_columns(y, affine, 10.0, out=y), repeats)
        for k in ("column_moments", "normalize_columns"):
            moved = n * d * 4 * (1 if k == "column_moments" else 2)
            row[k]["gb_per_s"] = round(moved / (row[k]["us_per_call"] * 1e-6) / 1e9, 1)
        out[name] = row
    r = torch.randn((T_FULL, N_ENVS), device="cuda", generator=g)
    dn = (torch.rand((T_FULL, N_ENVS), device="cuda", generator=g) < 1.0 / 800).to(torch.uint8)
    carry = torch.zeros(N_ENVS, device="cuda")
    trace = torch.empty_like(r)
    out["discounted_returns"] = dict(timed(lambda: ops.discounted_returns(r, dn, 0.99, carry, trace=trace), repeats), T=T_FULL, N=N_ENVS)
    return out


def bench_acting(T, repeats):
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.runner import create_net
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "discrete_action": False, "act_dim": 2,
           "image_batch": 1, "ped_sim": {"total": 3}}
    cfg = BaseConfig(types.SimpleNamespace(task="bench", ip="127.0.0.1"), env)
    cfg.TASK_TYPE = "robot_nav"
    net = create_net({"config": cfg, "config_nn": ConfigNN(env), "config_env": env}, max_batch=1024)
    shapes = [shape for _, shape in COMPONENTS]
    g = torch.Generator(device="cuda").manual_seed(7)
    obs = [torch.rand((T + 1, N_ENVS) + shape, device="cuda", generator=g) for shape in shapes]
    rew = torch.randn((T, N_ENVS), device="cuda", generator=g)
    dn = (torch.rand((T, N_ENVS), device="cuda", generator=g) < 1.0 / 800).to(torch.uint8)
    ros = {"off": StateRollout(net, N_ENVS, shapes, horizon=T),
           "on": StateRollout(net, N_ENVS, shapes, horizon=T, normalize_obs=True, normalize_returns=True)}

    def phase(ro):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(T + 1):
            ro.put_states(t, [o[t] for o in obs])
            if t < T:
                ro.act(t)
                ro.record(t, rew[t], dn[t])
        ro.bootstrap()
        ro.finish()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for ro in ros.values():
        phase(ro)  # warm-up
    times = {k: [] for k in ros}
    for _ in range(repeats):
        for k, ro in ros.items():  # interleaved: both see the same neighbours on the box
            times[k].append(phase(ro))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"envs": N_ENVS, "steps": T, "acting_ms_off": round(med["off"], 3), "acting_ms_on": round(med["on"], 3),
            "ms_per_step_off": round(med["off"] / (T + 1), 4), "ms_per_step_on": round(med["on"] / (T + 1), 4),
            "added_ms_per_step": round((med["on"] - med["off"]) / (T + 1), 4),
            "spread_ms_off": [round(min(times["off"]), 3), round(max(times["off"]), 3)],
            "spread_ms_on": [round(min(times["on"]), 3), round(max(times["on"]), 3)]}


def main():
    if not torch.cuda.is_available():
        sys.exit("bench_running_norm.py needs a GPU: a time taken elsewhere says nothing about it")
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    print(json.dumps({"workload": "running normalisation at the config-4 shapes", "ops": bench_ops(repeats), "acting": bench_acting(T, repeats)}))


if __name__ == "__main__":
    main()
