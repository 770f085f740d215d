#!/usr/bin/env python3
"""Generate tests/golden/f29_nav_status.npz by IMPORTING THE REFERENCE ITSELF (as make_golden.py does for F6, with its stubs).

Drives the reference's own Status.update_nav_status with float32 arrays on a seeded synthetic stream of info words (N = 24 envs, T = 400
steps, all_down with probability about 1/3; tests/nav_status_ref.py names the bits) and stores data only: the stream as packed words,
every per-env array of Status after steps 1, 3, 256 and 400, and what group_logger returns after the last step.  The stream is not a
trajectory of the env: a few steps that do not end an episode carry a goal bit or a collision kind, so that the rule "the running
episode's ring slot is overwritten by every step" is visible in the fixture.

Usage:  python tests/golden/make_golden_nav_status.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                               # tests/: nav_status_ref
sys.path.insert(0, HERE)

from make_golden import REF, _install_stubs  # noqa: E402
import nav_status_ref as S  # noqa: E402

N, T = 24, 400
CHECKPOINTS = (1, 3, 256, 400)
GROUP_CONFIG = {"env_type": "robot_nav", "ped_sim": {"total": 5}, "agent_num_per_env": 1}
REFERENCE_ARRAYS = tuple(k for k in S.PER_ENV if k != "trunc_num")       # trunc_num is this project's fifth ring


def make_stream(seed=29):
    rng = np.random.default_rng(seed)
    done = rng.random((T, N)) < 1 / 3
    done[:3, 0] = False                                                 # env 0 has finished nothing after step 3
    # the last finished episode of every env is steps 395..397: two close steps and one in the open, so every group_logger mean is finite
    done[394], done[395:397], done[397], done[398:] = True, False, True, False
    close = rng.random((T, N)) < 0.4
    close[395], close[396], close[397] = True, False, True
    how = rng.choice(6, size=(T, N), p=[0.3, 0.1, 0.1, 0.1, 0.2, 0.2])   # goal, wall, obstacle, wall + obstacle, pedestrian, time limit
    goal = done & (how == 0)
    wall = done & ((how == 1) | (how == 3))
    obstacle = done & ((how == 2) | (how == 3))
    kind = np.where(wall | obstacle, 1, np.where(done & (how == 4), 2, 0))
    trunc = done & (how == 5)
    stray = ~done & (rng.random((T, N)) < 0.08)                         # a running episode's slot that a later step overwrites
    stray_what = rng.integers(0, 3, size=(T, N))
    goal |= stray & (stray_what == 0)
    kind = np.where(stray & (stray_what > 0), stray_what, kind)
    v = rng.integers(0, 33, size=(T, N))
    w = rng.integers(-64, 65, size=(T, N))
    return S.pack_info(done, goal, kind, trunc, close, wall, obstacle, v, w)


def check_stream(words):
    """What the fixture has to cover (tests/test_nav_status_cpu.py asserts the same of the stored stream)."""
    f = S.unpack_info(words)
    done = f["done"] != 0
    assert words.shape == (T, N) and words.dtype == np.int32
    assert all(((f["collision"] == k) & done).any() for k in (1, 2)) and (f["goal"] & f["done"]).any() and f["truncated"].any()
    assert (f["close"] == 0).any() and (f["close"] == 1).any() and f["wall_hit"].any() and f["obstacle_hit"].any()
    assert done.sum(0).max() > S.WINDOW, "no ring wraps"
    assert (done[:3].sum(0) == 0).any() and (done.sum(0) >= 1).all()
    assert 0.28 < done.mean() < 0.39


def reference_info(words):
    """The info dict of one step as the reference's env wrappers hand it to Status: float32 arrays."""
    f = S.unpack_info(words)
    speeds = np.stack([f["v"].astype(np.float32) * np.float32(2.0 ** -5), f["w"].astype(np.float32) * np.float32(2.0 ** -6)], axis=1)
    return {"all_down": f["done"].astype(np.float32), "arrive": f["goal"].astype(np.float32), "collision": f["collision"].astype(np.int64),
            "speeds": speeds.astype(np.float32), "bool_get_close_to_human": f["close"].astype(np.float32),
            "is_clean": np.ones(len(words), np.float32)}


def main():
    _install_stubs()
    sys.path.insert(0, REF)
    from USTC_lab.agent.statistics import Status
    words = make_stream()
    check_stream(words)
    st = Status(N, np.float32, None)
    out = {"info": words, "checkpoints": np.array(CHECKPOINTS, np.int32)}
    for t in range(T):
        info = reference_info(words[t])
        st.update_nav_status(info, info["all_down"])
        if t + 1 in CHECKPOINTS:
            for k in REFERENCE_ARRAYS:
                a = np.asarray(getattr(st, k))
                assert a.dtype == (np.int32 if k == "episode_num" else np.float32), (k, a.dtype)
                out["c%d_%s" % (t + 1, k)] = a.copy()
    for k, v in st.group_logger(GROUP_CONFIG).items():
        if k != "ReducedRewardLogger":
            assert np.isfinite(v), k
            out["g_" + k] = np.float64(v)
    assert not st.coll_robot_num.any()
    path = os.path.join(HERE, "f29_nav_status.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
