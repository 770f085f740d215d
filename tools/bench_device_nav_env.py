#!/usr/bin/env python
"""What the device navigation env costs (env/device_nav_env.py, csrc/navenv.hip), on one box in one process, the
legs of each measurement alternating:

  (a) kernel   ddrl_op_nav_env_step for N envs against a plain device-to-device copy of the same N * 31,508 observation bytes -- what a
               rollout spends to take a ready-made device observation.  `calls` launches between one pair of device events give one
               sample (time per call); the samples of the two legs alternate.
  (b) acting   one rollout's acting phase on a StateRollout of BASELINE config 4's net (NavPreNet1D x2 + GaussionActor(2)), T steps
               between one pair of events: act -> env.step rendering into the pool rows -> record -> put_states_in_place, against the
               same phase on observations that are in the pool already (act -> record), and against the T act() calls and the T
               env.step calls alone.  env.step against act() at the same N is the comparison DESIGN.md reports.

  (c) info     ddrl_op_nav_env_step_info against ddrl_op_nav_env_step on two envs of the same seed under the same actions (DESIGN.md
               section 6.9), samples alternating as in (a).  The plain leg's samples are also split into its even and its odd ones: the
               gap between the two halves' medians is the session's own run-to-run spread, which the info leg is held against.
  (d) status   ddrl_op_nav_status_update over T x N info words and ddrl_op_nav_status_reduce, `calls` launches per sample.
  (e) final    ddrl_op_nav_env_step_final against ddrl_op_nav_env_step_info on envs of the same seed under the same actions (DESIGN.md
               section 6.12), at the env's default max_steps (truncations as rare as a fresh policy meets them) and at max_steps = 1
               (every env that does not collide truncates in every step: the terminal render at its most expensive), and the filing
               launch ddrl_op_file_flagged_rows of the terminal observations into pools of depth 1 under both.  The info leg's even and
               odd samples give the session's spread, as in (c).
  (f) bootstrap  the acting phase of (b) with the option on -- DeviceNavEnv(emit_final_obs=True), StateRollout(bootstrap_truncated=S),
               record() filing the rows -- against the same phase with it off, and finish() (with the extra forward) against finish().

  (g) ped_model  the step launch under the pedestrian models "walk" and "avoid"  in the plain, info and final
               forms, the six legs alternating, and "walk" through ddrl_op_nav_env_step_model against the entry that was there.

Every leg is warmed up first; a leg reports the median, the p95 and the extremes of its samples.  Prints one JSON line.

    python tools/bench_device_nav_env.py [--envs 512] [--steps 256] [--calls 200] [--samples 30] [--runs 10] [--warmup 2]
                                         [--ped-model walk] [--only LEGS]

--ped-model: the pedestrian model of every env of legs (a) to (f).  --only: a comma-separated subset of kernel, info, status, final,
acting, bootstrap, ped_model.
"""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_device_env import summary, timed  # noqa: E402

OBS_FLOATS = 960 + 5 + 3 * 48 * 48


def halves_spread(samples, **kw):
    """|median of the even samples - median of the odd ones| of one leg: the session's own run-to-run spread (None below two samples)."""
    if len(samples) < 2:
        return None
    a, b = (list(summary(samples[h::2], **kw).values())[0] for h in (0, 1))
    return round(abs(a - b), 4)


def make_net(max_batch, seed=0, **config_nn):
    """BASELINE config 4's net through create_net, as tools/bench_nav.py builds it; config_nn: ConfigNN fields to override."""
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.runner import create_net
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "discrete_action": False, "act_dim": 2, "image_batch": 1,
           "ped_sim": {"total": 3}}
    cfg = BaseConfig(types.SimpleNamespace(task="bench_device_nav_env", ip="127.0.0.1"), env)
    cfg.TASK_TYPE = "robot_nav"
    cfg_nn = ConfigNN(env)
    cfg_nn.SHARE_CNN_NET = False
    for name, value in config_nn.items():
        setattr(cfg_nn, name, value)
    torch.manual_seed(seed)
    return create_net({"config": cfg, "config_nn": cfg_nn, "config_env": env}, max_batch=max_batch)


def kernel_legs(args):
    from ddrl4nav_amd.env import DeviceNavEnv
    N = args.envs
    env = DeviceNavEnv(N, device="cuda", ped_model=args.ped_model, seed=1)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = torch.rand((N, 2), device="cuda", generator=g) * torch.tensor([1.0, 2.0], device="cuda") - torch.tensor([0.0, 1.0], device="cuda")
    src = torch.rand((N, OBS_FLOATS), device="cuda", generator=g)
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
    out["bytes_per_call"] = N * OBS_FLOATS * 4
    out["step_over_copy"] = round(out["env_step"]["median_us"] / out["d2d_copy"]["median_us"], 3)
    return out


def info_legs(args):
    from ddrl4nav_amd.env import DeviceNavEnv
    N = args.envs
    plain, told = DeviceNavEnv(N, device="cuda", ped_model=args.ped_model, seed=1), DeviceNavEnv(N, device="cuda", ped_model=args.ped_model, seed=1, emit_info=True)
    plain.reset()
    told.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = torch.rand((N, 2), device="cuda", generator=g) * torch.tensor([1.0, 2.0], device="cuda") - torch.tensor([0.0, 1.0], device="cuda")

    def leg(env):
        def run():
            for _ in range(args.calls):
                env.step(actions)
        return run

    legs = {"env_step": leg(plain), "env_step_info": leg(told)}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.samples):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    out = {k: summary(v, per=args.calls) for k, v in ms.items()}
    halves = [summary(ms["env_step"][h::2], per=args.calls)["median_us"] for h in (0, 1)]
    out["env_step_halves_median_us"] = halves
    out["env_step_spread_us"] = round(abs(halves[0] - halves[1]), 3)
    out["info_minus_plain_us"] = round(out["env_step_info"]["median_us"] - out["env_step"]["median_us"], 3)
    out["same_state"] = bool(torch.equal(plain.state, told.state))
    return out


def final_legs(args):
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.env import DeviceNavEnv
    N = args.envs
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = torch.rand((N, 2), device="cuda", generator=g) * torch.tensor([1.0, 2.0], device="cuda") - torch.tensor([0.0, 1.0], device="cuda")
    out = {}
    for name, max_steps in (("default_max_steps", 500), ("max_steps_1", 1)):
        told = DeviceNavEnv(N, device="cuda", ped_model=args.ped_model, seed=1, max_steps=max_steps, emit_info=True)
        final = DeviceNavEnv(N, device="cuda", ped_model=args.ped_model, seed=1, max_steps=max_steps, emit_final_obs=True)
        told.reset()
        final.reset()
        pools = [torch.zeros((1,) + tuple(f.shape), device="cuda") for f in final.final_obs]
        count = torch.zeros(N, dtype=torch.int32, device="cuda")
        slot = torch.zeros(N, dtype=torch.int32, device="cuda")
        truncated = torch.zeros((), dtype=torch.int64, device="cuda")

        def leg(env):
            def run():
                for _ in range(args.calls):
                    env.step(actions)
            return run

        def filing():                   # the info words and terminal rows the last step left; an empty pool every time
            for _ in range(args.calls):
                count.zero_()
                ops.file_flagged_rows(final.info, list(zip(final.final_obs, pools)), count, slot)

        def zeroing():                  # what the filing leg spends on emptying the pool
            for _ in range(args.calls):
                count.zero_()

        legs = {"env_step_info": leg(told), "env_step_final": leg(final), "file_flagged_rows_and_zero": filing, "zero_count": zeroing}
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(args.samples):
            for k, fn in legs.items():
                ms[k].append(timed(fn))
            truncated += ((final.info >> 4) & 1).sum()
        res = {k: summary(v, per=args.calls) for k, v in ms.items()}
        res["env_step_info_spread_us"] = halves_spread(ms["env_step_info"], per=args.calls)
        res["final_minus_info_us"] = round(res["env_step_final"]["median_us"] - res["env_step_info"]["median_us"], 3)
        res["filing_us"] = round(res["file_flagged_rows_and_zero"]["median_us"] - res["zero_count"]["median_us"], 3)
        res["truncated_share_of_last_steps"] = round(float(truncated) / (args.samples * N), 4)
        res["same_state"] = bool(torch.equal(told.state, final.state))
        out[name] = res
    return out


def bootstrap_legs(args):
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.env import DeviceNavEnv
    N, T = args.envs, args.steps
    net = make_net(N)
    plain = DeviceNavEnv(N, device="cuda", ped_model=args.ped_model, seed=1)
    final = DeviceNavEnv(N, device="cuda", ped_model=args.ped_model, seed=1, emit_final_obs=True)
    S = final.truncations_per_rollout(T)
    off = StateRollout(net, N, plain.state_shapes, horizon=T)
    on = StateRollout(net, N, final.state_shapes, horizon=T, bootstrap_truncated=S)
    for env, ro in ((plain, off), (final, on)):
        env.reset(obs_out=ro.state_rows(0))
        ro.put_states_in_place(0)

    def acting_off():
        for t in range(T):
            _, r, d = plain.step(off.act(t), obs_out=off.state_rows(t + 1))
            off.record(t, r, d)
            off.put_states_in_place(t + 1)

    def acting_on():
        on.trunc_count.zero_()
        for t in range(T):
            _, r, d = final.step(on.act(t), obs_out=on.state_rows(t + 1))
            on.record(t, r, d, info=final.info, final_obs=final.final_obs)
            on.put_states_in_place(t + 1)

    legs = {"acting_off": acting_off, "acting_on": acting_on, "finish_off": off.finish, "finish_on": on.finish}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.runs):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    out = {k: summary(v, unit="ms") for k, v in ms.items()}
    out["acting_off_spread_ms"] = halves_spread(ms["acting_off"], unit="ms")
    out["acting_on_over_off"] = round(out["acting_on"]["median_ms"] / out["acting_off"]["median_ms"], 4)
    out["finish_on_minus_off_ms"] = round(out["finish_on"]["median_ms"] - out["finish_off"]["median_ms"], 4)
    out["S"] = S
    out["truncations_dropped"] = on.truncations_dropped()
    return out


def ped_model_legs(args):
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.env import DeviceNavEnv
    N = args.envs
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = torch.rand((N, 2), device="cuda", generator=g) * torch.tensor([1.0, 2.0], device="cuda") - torch.tensor([0.0, 1.0], device="cuda")
    forms = {"plain": {}, "info": dict(emit_info=True), "final": dict(emit_final_obs=True)}
    envs = {"%s_%s" % (model, form): DeviceNavEnv(N, device="cuda", seed=1, ped_model=model, **kw)
            for form, kw in forms.items() for model in ("walk", "avoid")}
    for env in envs.values():
        env.reset()
    through = DeviceNavEnv(N, device="cuda", seed=1)       # "walk" through the entry point that takes the model
    through.reset()

    def leg(env):
        def run():
            for _ in range(args.calls):
                env.step(actions)
        return run

    def walk_through_model():
        for _ in range(args.calls):
            ops.nav_env_step_model(through.state, actions, through.obs, through.reward, through.done, ped_model="walk", seed=1)

    legs = {k: leg(env) for k, env in envs.items()}
    legs["walk_plain_through_step_model"] = walk_through_model
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.samples):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    out = {k: summary(v, per=args.calls) for k, v in ms.items()}
    for form in forms:
        w, a = "walk_%s" % form, "avoid_%s" % form
        out[w]["spread_us"] = halves_spread(ms[w], per=args.calls)
        out[a]["over_walk"] = round(out[a]["median_us"] / out[w]["median_us"], 4)
        out[a]["minus_walk_us"] = round(out[a]["median_us"] - out[w]["median_us"], 3)
    out["same_state_walk"] = bool(torch.equal(envs["walk_plain"].state, envs["walk_final"].state)
                                  and torch.equal(envs["walk_plain"].state, through.state))
    out["same_state_avoid"] = bool(torch.equal(envs["avoid_plain"].state, envs["avoid_final"].state))
    return out


def status_legs(args):
    from ddrl4nav_amd.agent import NavStatus
    N, T = args.envs, args.steps
    g = torch.Generator(device="cuda").manual_seed(2)
    done = (torch.rand((T, N), device="cuda", generator=g) < 0.02).to(torch.int32)
    close = (torch.rand((T, N), device="cuda", generator=g) < 0.3).to(torch.int32)
    v = torch.randint(0, 33, (T, N), device="cuda", generator=g, dtype=torch.int32)
    w = torch.randint(0, 129, (T, N), device="cuda", generator=g, dtype=torch.int32)
    info = (done | (done << 1) | (close << 5) | (v << 8) | (w << 16)).contiguous()
    st = NavStatus(N, "cuda")

    def updates():
        for _ in range(args.calls):
            st.update(info)

    def reduces():
        for _ in range(args.calls):
            st.partial()

    legs = {"status_update": updates, "status_reduce": reduces}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.samples):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    return {k: summary(v, per=args.calls) for k, v in ms.items()}


def acting_legs(args):
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.env import DeviceNavEnv
    N, T = args.envs, args.steps
    net = make_net(N)
    env = DeviceNavEnv(N, device="cuda", ped_model=args.ped_model, seed=1)
    ro = StateRollout(net, N, env.state_shapes, horizon=T)
    env.reset(obs_out=ro.state_rows(0))
    ro.put_states_in_place(0)

    def with_env():
        for t in range(T):
            _, r, d = env.step(ro.act(t), obs_out=ro.state_rows(t + 1))
            ro.record(t, r, d)
            ro.put_states_in_place(t + 1)

    def in_pool():                      # the observations the env left in the pool, its last reward and done
        for t in range(T):
            ro.act(t)
            ro.record(t, env.reward, env.done)

    def act_only():
        for t in range(T):
            ro.act(t)

    def env_only():
        for t in range(T):
            env.step(ro._actions[t], obs_out=ro.state_rows(t + 1))

    legs = {"device_env": with_env, "observations_in_pool": in_pool, "act_only": act_only, "env_step_only": env_only}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.runs):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    out = {k: summary(v, unit="ms") for k, v in ms.items()}
    out["device_env_over_in_pool"] = round(out["device_env"]["median_ms"] / out["observations_in_pool"]["median_ms"], 4)
    out["env_step_over_act"] = round(out["env_step_only"]["median_ms"] / out["act_only"]["median_ms"], 4)
    out["env_steps_per_s_device_env"] = round(N * T / (out["device_env"]["median_ms"] / 1000.0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--calls", type=int, default=200, help="launches per sample of the kernel legs")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--runs", type=int, default=10, help="timed acting phases per leg")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ped-model", choices=("walk", "avoid"), default="walk", help="the pedestrian model of the envs of legs (a) to (f)")
    ap.add_argument("--only", default=None, help="comma-separated legs to run (default: all)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_device_nav_env needs a GPU: there is nothing to measure without one")
    legs = {"kernel": kernel_legs, "info": info_legs, "status": status_legs, "final": final_legs, "acting": acting_legs,
            "bootstrap": bootstrap_legs, "ped_model": ped_model_legs}
    only = list(legs) if args.only is None else args.only.split(",")
    if any(k not in legs for k in only):
        sys.exit("--only takes a comma-separated subset of %s" % ", ".join(legs))
    out = {"tool": "bench_device_nav_env", "N": args.envs, "T": args.steps, "ped_model": args.ped_model,
           "device": torch.cuda.get_device_name(0)}
    for k in only:
        out[k] = legs[k](args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
