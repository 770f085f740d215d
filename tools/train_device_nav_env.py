#!/usr/bin/env python
"""Train BASELINE config 4's net (NavPreNet1D x2 + GaussionActor(2)) on the device navigation env (env/device_nav_env.py; DESIGN.md
section 6.8): the whole loop -- acting, the env, GAE, the update -- on one GPU through runner/device_loop.train_states.  Writes the
mean-return curve as JSON: per update the env steps so far, the mean return of the envs' latest finished episodes
(EpisodeReturns.mean_return) and the last loss dict of the update; next to it the return of the uniform-random policy (a0 ~ U(0, 1),
a1 ~ U(-1, 1)) on the same env, measured first on the device over --baseline-steps steps.

    python tools/train_device_nav_env.py [--envs 256] [--horizon 64] [--updates 100] [--obstacles 10] [--peds 5] [--max-steps 500]
                                         [--iters 4] [--actor-lr R] [--critic-lr R] [--normalize-obs] [--seed 0] [--out curve.json]
                                         [--nav-status] [--robots 1] [--dagger ITERS] [--ped-model walk]

--nav-status: the env emits its info words and the rollout keeps the reference's navigation statistics on the device (agent.NavStatus;
DESIGN.md section 6.9); reach, collision and truncation rates over the envs' latest 100 episodes are printed next to the return and
stored in the curve.  The loop gains no host synchronisation per step: the one copy is NavStatus.summary() at a logged update.

--robots R (2..4): --envs counts WORLDS of R robots each (env/fleet_nav_env.py) and the rollout has envs * R rows,
one per robot; with --nav-status the other-robot collision rate (NavStatus.other_robot_collision_rate, one more scalar copy at a logged
update) is printed and stored too.  --robots 1 is the single-robot env above.

--dagger ITERS (default 0: off, and nothing below runs): ahead of the PPO updates, ITERS rounds of DAgger (runner/dagger_loop.py; DESIGN.md
section 6.15) -- the net acts, the scripted expert (env.NavExpert) labels every visited state, GenericPPO.clone_actor fits the actor;
beta goes from 1 to 0.  With --nav-status the net's mean action is played for --baseline-steps steps before and after, from the same
reset, and the two reach rates are printed and stored: whether cloning helped is a measurement, not a claim.

--ped-model avoid: the pedestrians give way to each other and to the robots instead of walking straight ahead;
it goes with every option above.  The scripted expert of --dagger still predicts pedestrians that walk straight ahead.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_device_nav_env import make_net  # noqa: E402


def random_policy_return(env, steps, seed):
    """(mean return per finished episode, mean reward per env per 1,000 steps) of uniform-random actions; leaves the env reset."""
    g = torch.Generator(device=env.device).manual_seed(seed)
    scale, shift = torch.tensor([1.0, 2.0], device=env.device), torch.tensor([0.0, 1.0], device=env.device)
    env.reset()
    total = torch.zeros((), dtype=torch.float64, device=env.device)
    episodes = torch.zeros((), dtype=torch.float64, device=env.device)
    for _ in range(steps):
        _, r, d = env.step(torch.rand((env.N, 2), device=env.device, generator=g) * scale - shift)
        total += r.sum()
        episodes += d.sum()
    env.reset()
    total, episodes = float(total.item()), float(episodes.item())
    return (total / episodes if episodes else float("nan")), 1000.0 * total / (env.N * steps)


def policy_outcomes(net, env, steps):
    """The outcomes of the net's mean action over `steps` steps from a reset, read off the info words (the env needs emit_info):
    {episodes, reach_rate, collision_rate, truncation_rate}; leaves the env reset."""
    obs = env.reset()
    counts = torch.zeros(4, dtype=torch.int64, device=env.device)
    for _ in range(steps):
        with torch.no_grad():
            (mu, _), _ = net.forward(obs, None, True)
        obs = env.step(mu)[0]
        w = env.info
        counts += torch.stack([(w & 1).sum(), ((w >> 1) & 1).sum(), (((w >> 2) & 3) != 0).sum(), ((w >> 4) & 1).sum()])
    env.reset()
    done, goal, hit, trunc = (int(c) for c in counts.tolist())
    rate = lambda k: k / done if done else float("nan")
    return {"episodes": done, "reach_rate": rate(goal), "collision_rate": rate(hit), "truncation_rate": rate(trunc)}


def run_dagger(args, net, env, out):
    from ddrl4nav_amd.data import DemoPool
    from ddrl4nav_amd.env import NavExpert
    from ddrl4nav_amd.runner import dagger_loop
    if args.robots > 1:
        sys.exit("--dagger is built for the single-robot env: a FleetNavEnv has no expert")
    log = out["dagger"] = {"iterations": args.dagger, "steps": args.dagger_steps, "lr": args.dagger_lr, "batch": args.dagger_batch,
                           "epochs": args.dagger_epochs, "rounds": []}
    if args.nav_status:
        log["before"] = policy_outcomes(net, env, args.baseline_steps)
        print("before cloning: %s" % log["before"], flush=True)
    pool = DemoPool(env.state_shapes, 2, env.N * max(2, args.dagger_pool), device=net.device, n_envs=env.N)
    t0 = time.time()
    rounds = dagger_loop.run(net, env, NavExpert(env), pool, args.dagger, args.dagger_steps, lr=args.dagger_lr, batch=args.dagger_batch,
                             epochs=args.dagger_epochs, seed=args.seed)
    for i, (loss, beta) in enumerate(rounds, 1):
        log["rounds"].append({"round": i, "beta": beta, "mean_clone_loss": loss, "rows": len(pool)})
        print("dagger %3d  beta %.2f  rows %7d  mean clone loss %.5f  %.0f s" % (i, beta, len(pool), loss, time.time() - t0), flush=True)
    if args.nav_status:
        log["after"] = policy_outcomes(net, env, args.baseline_steps)
        print("after cloning:  %s" % log["after"], flush=True)
    env.reset()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--obstacles", type=int, default=10)
    ap.add_argument("--peds", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=500)
    ap.add_argument("--iters", type=int, default=4, help="TRAINING_ITER_TIME: passes over a rollout's batch")
    ap.add_argument("--micro-batch", type=int, default=4096, help="the net's max_batch: samples per launch of the update")
    ap.add_argument("--actor-lr", type=float, default=None)
    ap.add_argument("--critic-lr", type=float, default=None)
    ap.add_argument("--normalize-obs", action="store_true", help="StateRollout(normalize_obs=True)")
    ap.add_argument("--nav-status", action="store_true", help="track and print reach / collision / truncation rates (agent.NavStatus)")
    ap.add_argument("--bootstrap-truncated", action="store_true",
                    help="GAE goes on from the critic's value of a truncated episode's last observation (DESIGN.md section 6.12): the "
                         "env renders it, StateRollout(bootstrap_truncated=env.truncations_per_rollout(horizon)) files and evaluates it")
    ap.add_argument("--robots", type=int, default=1, help="robots per world; above 1 the env is a FleetNavEnv and --envs counts worlds")
    ap.add_argument("--ped-model", choices=("walk", "avoid"), default="walk",
                    help="avoid: pedestrians that give way to each other and to the robots (DESIGN.md section 6.16)")
    ap.add_argument("--dagger", type=int, default=0, help="rounds of DAgger ahead of the PPO updates (0: off)")
    ap.add_argument("--dagger-steps", type=int, default=64, help="env steps collected per round")
    ap.add_argument("--dagger-pool", type=int, default=256, help="the demonstration pool's depth in steps (rows = envs x this)")
    ap.add_argument("--dagger-lr", type=float, default=3e-4)
    ap.add_argument("--dagger-batch", type=int, default=1024)
    ap.add_argument("--dagger-epochs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--baseline-steps", type=int, default=1000)
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--out", default=None, help="the curve as JSON (default: printed only)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_device_nav_env needs a GPU")

    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.env import make_device_env
    from ddrl4nav_amd.runner.device_loop import train_states

    knobs = {"TRAINING_ITER_TIME": args.iters}
    for name, value in (("ACTOR_LEARNING_RATE", args.actor_lr), ("CRITIC_LEARNING_RATE", args.critic_lr)):
        if value is not None:
            knobs[name] = value
    if args.robots < 1:
        sys.exit("--robots must be at least 1")
    rows = args.envs * args.robots
    net = make_net(max(args.micro_batch, rows), seed=args.seed, **knobs)
    config_env = {"env_name": "DeviceNav-v0", "env_num": args.envs, "env_seed": args.seed, "env_obstacles": args.obstacles,
                  "env_peds": args.peds, "env_max_steps": args.max_steps, "env_info": args.nav_status,
                  "env_final_obs": args.bootstrap_truncated, "env_ped_model": args.ped_model}
    if args.robots > 1:
        config_env.update(env_name="DeviceNavFleet-v0", agent_num_per_env=args.robots)
    env = make_device_env(config_env, device=net.device)
    ro = StateRollout(net, env.N, env.state_shapes, horizon=args.horizon, track_returns=True, normalize_obs=args.normalize_obs or None,
                      track_nav_status=args.nav_status,
                      bootstrap_truncated=env.truncations_per_rollout(args.horizon) if args.bootstrap_truncated else 0)

    per_episode, per_1000 = random_policy_return(env, args.baseline_steps, args.seed + 1)
    out = {"tool": "train_device_nav_env", "N": rows, "robots": args.robots, "T": args.horizon, "obstacles": args.obstacles, "peds": args.peds,
           "ped_model": args.ped_model, "max_steps": args.max_steps, "iters": args.iters, "normalize_obs": bool(args.normalize_obs),
           "bootstrap_truncated": ro.S,
           "device": torch.cuda.get_device_name(0),
           "random_policy": {"return_per_episode": per_episode, "reward_per_env_per_1000_steps": per_1000, "steps": args.baseline_steps},
           "curve": []}
    print("random policy: %.3f per episode, %.2f per env per 1,000 steps" % (per_episode, per_1000), flush=True)
    if args.dagger > 0:
        run_dagger(args, net, env, out)
    t0 = time.time()
    for u, (losses, mean_return) in enumerate(train_states(net, env, ro, args.updates), 1):
        out["curve"].append({"update": u, "env_steps": u * rows * args.horizon, "mean_return": mean_return,
                             "losses": {k: v for k, v in losses.items() if k != "PpoBackUpTime"}})
        if u % args.log_every == 0 or u == args.updates:
            rates = ""
            if ro.nav_status is not None:
                status = ro.nav_status.summary()
                out["curve"][-1]["nav_status"] = status
                rates = "  reach %.3f  static %.3f  ped %.3f  trunc %.3f" % tuple(
                    status[k] for k in ("ReducedReachRateLogger", "ReducedStaticObsCollisionRateLogger", "ReducedPedCollisionRateLogger",
                                        "TruncationRate"))
                if args.robots > 1:
                    status["ReducedOtherRobotCollisionRateLogger"] = ro.nav_status.other_robot_collision_rate()
                    rates += "  robot %.3f" % status["ReducedOtherRobotCollisionRateLogger"]
            print("update %4d  steps %9d  mean return %8.3f%s  VLoss %.4f  EntLoss %.4f  %.0f s"
                  % (u, u * rows * args.horizon, mean_return, rates, losses["VLoss"], losses["EntLoss"], time.time() - t0), flush=True)
    out["seconds"] = round(time.time() - t0, 1)
    out["env_steps_per_s_end_to_end"] = round(args.updates * rows * args.horizon / max(out["seconds"], 1e-9))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)
    brief = {k: v for k, v in out.items() if k != "curve"}
    brief["first_return"] = next((c["mean_return"] for c in out["curve"] if c["mean_return"] == c["mean_return"]), None)
    brief["last_return"] = out["curve"][-1]["mean_return"] if out["curve"] else None
    if ro.nav_status is not None and out["curve"]:
        brief["last_nav_status"] = out["curve"][-1].get("nav_status")
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
