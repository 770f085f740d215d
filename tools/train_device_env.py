#!/usr/bin/env python
"""Train the Atari PPO net on a device env (env/device_env.py): the whole loop -- acting, the env, GAE, the
update -- on one GPU through runner/device_loop.train.  Writes the mean-return curve as JSON: per update the env steps so far, the
mean return of the envs' latest finished episodes (EpisodeReturns.mean_return) and the last loss dict of the update; next to it the
return of the uniform-random policy on the same env, measured first on the device over --baseline-steps steps.

    python tools/train_device_env.py --game catch|pong [--envs 256] [--horizon 64] [--updates 200] [--share] [--out curve.json]
                                     [--points 21] [--max-steps 10000] [--iters 4] [--minibatches 4] [--entropy 0.01] [--entropy-split]
                                     [--actor-lr R] [--critic-lr R] [--lr R] [--seed 0]
"""
import argparse
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, A = 4, 6


def random_policy_return(env, steps, seed):
    """(mean return per finished episode, mean reward per env per 1,000 steps) of uniform-random actions; leaves the env reset."""
    g = torch.Generator(device=env.device).manual_seed(seed)
    env.reset()
    total = torch.zeros((), dtype=torch.float64, device=env.device)
    episodes = torch.zeros((), dtype=torch.float64, device=env.device)
    for _ in range(steps):
        _, r, d = env.step(torch.randint(0, env.n_actions, (env.N,), device=env.device, generator=g).to(torch.float32))
        total += r.sum()
        episodes += d.sum()
    env.reset()
    total, episodes = float(total.item()), float(episodes.item())
    return (total / episodes if episodes else float("nan")), 1000.0 * total / (env.N * steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", choices=("pong", "catch"), required=True)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--share", action="store_true", help="SHARE_CNN_NET = True: one encoder for both heads")
    ap.add_argument("--points", type=int, default=21)
    ap.add_argument("--max-steps", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=4, help="TRAINING_ITER_TIME: passes over a rollout's batch")
    ap.add_argument("--minibatches", type=int, default=4, help="PPO_MINIBATCHES")
    ap.add_argument("--entropy", type=float, default=0.01, help="ENTROPY_LOSS_THETA")
    ap.add_argument("--entropy-split", action="store_true",
                    help="ENTROPY_BONUS_SPLIT: with two encoders the entropy coefficient reaches the actor only with it")
    ap.add_argument("--actor-lr", type=float, default=None)
    ap.add_argument("--critic-lr", type=float, default=None)
    ap.add_argument("--lr", type=float, default=None, help="LEARNING_RATE of the shared-encoder mode")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--baseline-steps", type=int, default=2000)
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--out", default=None, help="the curve as JSON (default: printed only)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_device_env needs a GPU")

    from ddrl4nav_amd.agent import PlaneRollout
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.env import make_device_env
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.runner.device_loop import train

    cfg_env = {"env_type": "gym", "env_name": {"pong": "DevicePong-v0", "catch": "DeviceCatch-v0"}[args.game], "env_num": args.envs,
               "int_frame_stack": C, "discrete_action": True, "discrete_actions": list(range(A)), "agent_num_per_env": 1,
               "batch_num_per_env": 8, "env_seed": args.seed, "env_points": args.points, "env_max_steps": args.max_steps}
    cfg_nn = ConfigNN(cfg_env)
    cfg_nn.SHARE_CNN_NET = bool(args.share)
    cfg_nn.TRAINING_ITER_TIME = args.iters
    cfg_nn.PPO_MINIBATCHES = args.minibatches
    cfg_nn.PPO_SHUFFLE = args.minibatches > 1
    cfg_nn.NORMALIZE_ADVANTAGE = "batch"
    cfg_nn.ENTROPY_LOSS_THETA = args.entropy
    cfg_nn.ENTROPY_BONUS_SPLIT = bool(args.entropy_split)
    for name, value in (("ACTOR_LEARNING_RATE", args.actor_lr), ("CRITIC_LEARNING_RATE", args.critic_lr), ("LEARNING_RATE", args.lr)):
        if value is not None:
            setattr(cfg_nn, name, value)
    torch.manual_seed(args.seed)
    cfg = BaseConfig(types.SimpleNamespace(task="train_device_env", ip="127.0.0.1"), dict(cfg_env, env_name="PongNoFrameskip-v4"))
    net = create_net({"config": cfg, "config_nn": cfg_nn, "config_env": cfg_env}, max_batch=args.envs * args.horizon)
    env = make_device_env(cfg_env, device=net.device)
    ro = PlaneRollout(net, args.envs, horizon=args.horizon, channels=C, seed=args.seed, track_returns=True)

    per_episode, per_1000 = random_policy_return(env, args.baseline_steps, args.seed + 1)
    out = {"tool": "train_device_env", "game": args.game, "N": args.envs, "T": args.horizon, "share_cnn_net": bool(args.share),
           "points": args.points, "max_steps": args.max_steps, "iters": args.iters, "minibatches": args.minibatches,
           "device": torch.cuda.get_device_name(0),
           "random_policy": {"return_per_episode": per_episode, "reward_per_env_per_1000_steps": per_1000, "steps": args.baseline_steps},
           "curve": []}
    print("random policy: %.3f per episode, %.2f per env per 1,000 steps" % (per_episode, per_1000), flush=True)
    t0 = time.time()
    for u, (losses, mean_return) in enumerate(train(net, env, ro, args.updates), 1):
        out["curve"].append({"update": u, "env_steps": u * args.envs * args.horizon, "mean_return": mean_return,
                             "losses": {k: v for k, v in losses.items() if k != "PpoBackUpTime"}})
        if u % args.log_every == 0 or u == args.updates:
            print("update %4d  steps %9d  mean return %8.3f  VLoss %.4f  EntLoss %.4f  %.0f s"
                  % (u, u * args.envs * args.horizon, mean_return, losses["VLoss"], losses["EntLoss"], time.time() - t0), flush=True)
    out["seconds"] = round(time.time() - t0, 1)
    out["env_steps_per_s_end_to_end"] = round(args.updates * args.envs * args.horizon / max(out["seconds"], 1e-9))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f)
    brief = {k: v for k, v in out.items() if k != "curve"}
    brief["first_return"] = next((c["mean_return"] for c in out["curve"] if c["mean_return"] == c["mean_return"]), None)
    brief["last_return"] = out["curve"][-1]["mean_return"] if out["curve"] else None
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
