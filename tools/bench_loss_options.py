#!/usr/bin/env python3
"""Event time of the loss block with and without the update options: the `heads_loss` span of a whole PPO
iteration of the Atari context (the loss kernel and its partial reduce, as ddrl_profile_enable brackets them) at B = 65,536, the plain
kernel against its option instantiation with the value clip, the split entropy bonus and both.  The variants alternate inside one
process; per variant the median, minimum and maximum of `--runs` iterations.  A report, not a gate.

    python tools/bench_loss_options.py [--batch 65536] [--runs 20] [--warmup 3] [--actions 6] [--shared 0]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = (("plain", (0.0, False)), ("clip", (0.2, False)), ("entropy", (0.0, True)), ("both", (0.2, True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--actions", type=int, default=6)
    ap.add_argument("--shared", type=int, default=0)
    args = ap.parse_args()
    from ddrl4nav_amd.engine import HotPath
    from ddrl4nav_amd.utils.recipe import flatten, make_weights
    B, A = args.batch, args.actions
    hp = HotPath(max_batch=B, n_actions=A, share_cnn_net=args.shared)
    hp.set_params(flatten(make_weights(0, n_actions=A, shared=bool(args.shared)), n_actions=A, shared=bool(args.shared)))
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    rng = np.random.default_rng(0)
    d = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    cols = [d(rng.integers(0, A, size=B)), d(np.full(B, -np.log(A)) + rng.normal(0, 0.3, B)), d(rng.normal(size=B)), d(rng.normal(size=B))]
    old_values = d(rng.normal(size=B))
    hp.profile(True, acting=False)
    seen = {}

    def heads_loss_ms():
        """this iteration's share of the accumulated `heads_loss` span"""
        ms, calls = hp.profile_read()["heads_loss"]
        last = seen.get("t", (0.0, 0))
        seen["t"] = (ms, calls)
        assert calls == last[1] + 1
        return ms - last[0]

    times = {name: [] for name, _ in VARIANTS}
    for r in range(args.warmup + args.runs):
        for name, options in VARIANTS:
            hp.loss_options = options
            hp.ppo_iter(frames, *cols, old_values=old_values)
            t = heads_loss_ms()
            if r >= args.warmup:
                times[name].append(t)
    hp.close()
    out = {"batch": B, "actions": A, "shared": args.shared, "runs": args.runs}
    for name, _ in VARIANTS:
        t = times[name]
        out[name] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
        print("%-8s heads_loss median %.4f ms  min %.4f  max %.4f  (x %.3f of plain)" % (
            name, out[name]["median_ms"], out[name]["min_ms"], out[name]["max_ms"],
            out[name]["median_ms"] / max(out["plain"]["median_ms"], 1e-9)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
