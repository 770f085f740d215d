#!/usr/bin/env python3
"""Acting phase with the frames crossing PCIe, whole stacks against single frames.  Not the headline bench
(bench.py is, and it keeps the frames resident); prints one JSON line.

One rollout = T + 1 ring slots popped into the device pool, T acting forwards and the bootstrap forward (default Pong net, 256 envs,
T = 256, C = 4; synthetic frames from numpy.random.default_rng(1234)).  Four legs, interleaved A B C D A B C D in one process:
  full_serial     DeviceRollout.put_frames_from_ring       (N*C*7056 bytes per step), the host waits for every copy and every forward
  single_serial   DeviceRollout.put_new_frames_from_ring   (N*7056 bytes per step + the push kernel), the same waits
  full_overlap    put_frames_from_ring, no host wait: the producer thread runs ahead, copy t + 1 runs under forward t
  single_overlap  put_new_frames_from_ring, no host wait
The producer commits slots that already hold frames (env workers write into the pinned slots themselves, as bench.py's ingest leg).
Median and p95 of the wall-clock milliseconds per rollout over --rollouts measured rollouts per leg, after --warmup unmeasured ones.

Usage: python tools/bench_ingest_frames.py [--envs 256] [--steps 256] [--channels 4] [--rollouts 20] [--warmup 3]"""
import argparse
import json
import os
import sys
import threading
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddrl4nav_amd.agent import DeviceRollout  # noqa: E402
from ddrl4nav_amd.config import BaseConfig, ConfigNN  # noqa: E402
from ddrl4nav_amd.data import PinnedRing  # noqa: E402
from ddrl4nav_amd.runner import create_net  # noqa: E402

PLANE = 84 * 84
LEGS = ("full_serial", "single_serial", "full_overlap", "single_overlap")
RING_SLOTS = 16


def build_net(n_envs, horizon, channels):
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": n_envs, "int_frame_stack": channels,
           "discrete_action": True, "discrete_actions": list(range(6)), "agent_num_per_env": 1, "batch_num_per_env": n_envs}
    config = BaseConfig(types.SimpleNamespace(task="bench", ip="127.0.0.1"), env)
    config.TIME_MAX = horizon
    return create_net({"config": config, "config_nn": ConfigNN(env), "config_env": env}, max_batch=max(n_envs, 128))


def filled_ring(rng, slot_bytes, device):
    """A ring whose every slot holds random frames before the clock starts."""
    ring = PinnedRing(slot_bytes, n_slots=RING_SLOTS)
    for _ in range(RING_SLOTS):
        buf = ring.acquire(timeout_ms=10000)
        buf[:] = rng.integers(0, 256, size=slot_bytes, dtype=np.uint8)
        ring.commit()
    scratch = torch.empty(slot_bytes, dtype=torch.uint8, device=device)
    for _ in range(RING_SLOTS):
        ring.pop_to(scratch)
    torch.cuda.synchronize()
    return ring


def rollout_ms(ro, ring, single, serial):
    """Wall-clock milliseconds of one acting phase fed from `ring` by a producer thread."""
    T = ro.T
    err = []

    def producer():
        try:
            for _ in range(T + 1):
                ring.acquire(timeout_ms=30000)
                ring.commit()
        except Exception as e:  # surfaced below; the consumer's pop times out
            err.append(e)

    th = threading.Thread(target=producer, daemon=True)
    th.start()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(T + 1):
        if single:
            ro.put_new_frames_from_ring(t, ring, reset=True if t == 0 else None)
        else:
            ro.put_frames_from_ring(t, ring)
        if serial:
            torch.cuda.synchronize()
        ro.act(t)          # t == T: the bootstrap forward
        if serial:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    th.join(30)
    if err or th.is_alive():
        raise RuntimeError("ring producer failed: %r" % (err[0] if err else "still running"))
    ro.finish()            # untimed: closes the rollout (GAE on the pool), as a host would before the next one
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=256, help="T: acting steps per rollout")
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--rollouts", type=int, default=20, help="measured rollouts per leg")
    ap.add_argument("--warmup", type=int, default=3, help="unmeasured rollouts per leg")
    args = ap.parse_args()
    N, T, C = args.envs, args.steps, args.channels
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    net = build_net(N, T, C)
    ro = DeviceRollout(net, N, horizon=T, channels=C, seed=0)
    rng = np.random.default_rng(1234)
    ro.dones.copy_(torch.from_numpy((rng.random((T, N)) < 1.0 / 800).astype(np.uint8)))
    nbytes = {"full": N * C * PLANE, "single": N * PLANE}
    rings = {k: filled_ring(rng, v, dev) for k, v in nbytes.items()}
    ms = {leg: [] for leg in LEGS}
    for r in range(args.warmup + args.rollouts):
        for leg in LEGS:
            kind, mode = leg.split("_")
            x = rollout_ms(ro, rings[kind], single=kind == "single", serial=mode == "serial")
            if r >= args.warmup:
                ms[leg].append(x)
    for ring in rings.values():
        ring.close()

    out = {"metric": "acting phase of one rollout, frames through the pinned ring", "unit": "ms per rollout (wall clock)",
           "gpu": torch.cuda.get_device_name(0), "envs": N, "steps": T, "channels": C, "rollouts": args.rollouts, "warmup": args.warmup,
           "order": "interleaved: " + " ".join(LEGS)}
    for leg in LEGS:
        a = np.asarray(ms[leg])
        med, p95 = float(np.median(a)), float(np.percentile(a, 95))
        out[leg] = {"median_ms": round(med, 3), "p95_ms": round(p95, 3), "spread_ms": round(p95 - med, 3),
                    "min_ms": round(float(a.min()), 3), "us_per_step": round(med * 1e3 / (T + 1), 2),
                    "env_steps_per_s": round(N * T / (med * 1e-3), 1), "bytes_per_step": nbytes[leg.split("_")[0]]}
    # the claims of DESIGN.md section 5, against the full-stack legs of THIS run: the spread is the larger (p95 - median) of the pair
    for mode in ("serial", "overlap"):
        f, s = out["full_" + mode], out["single_" + mode]
        spread = max(f["spread_ms"], s["spread_ms"])
        out[mode + "_compare"] = {"single_minus_full_ms": round(s["median_ms"] - f["median_ms"], 3), "spread_ms": spread,
                                  "single_faster_beyond_spread": bool(f["median_ms"] - s["median_ms"] > spread),
                                  "single_not_slower_beyond_spread": bool(s["median_ms"] - f["median_ms"] <= spread)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
