#!/usr/bin/env python3
"""Generate tests/golden/f28_running_mean_std.npz by IMPORTING THE REFERENCE's RunningMeanStd
(USTC_lab/env/gym_env/wrapper/warputils.py:83-109), the class the reference defines and uses nowhere.

Runs only where the reference is checked out (DDRL_REFERENCE, read-only).  Nothing of it is copied: the script drives the reference's
own class on seeded inputs and stores inputs + outputs as arrays.  warputils.py imports ``gym`` and ``cv2`` at module level (its env
wrappers subclass gym.Wrapper); both are absent from the image and are stubbed in-process, the way make_golden.py stubs ``redis`` --
RunningMeanStd touches neither.  The package __init__ files above warputils.py import the env factories (and through them the
simulators), so the parent packages are entered as bare namespace modules and only warputils.py itself is executed.

The fixture: six updates of one RunningMeanStd over d = 5 features with batch sizes 1, 2, 7, 64, 3, 513.  The batches are float64
arrays whose values are exactly representable in float32 (the device kernels read the same numbers as fp32); the columns differ in
offset and scale, |mean| / std <= 100.  After every update: count, mean[5], var[5].

Usage:  python tests/golden/make_golden_running_norm.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DDRL_REFERENCE", "/root/reference")
BATCHES = (1, 2, 7, 64, 3, 513)
D = 5
OFFSET = np.array([0.0, 3.5, -120.0, 0.25, 40.0])     # metres, a goal vector, a far range: columns of different units
SCALE = np.array([1.0, 0.05, 2.0, 30.0, 0.5])


def _install_stubs():
    class _Base:
        def __init__(self, *a, **k):
            pass

    gym = types.ModuleType("gym")
    for name in ("Wrapper", "ObservationWrapper", "RewardWrapper", "ActionWrapper", "Env"):
        setattr(gym, name, type(name, (_Base,), {}))
    gym.spaces = types.ModuleType("gym.spaces")
    gym.spaces.Box = gym.spaces.Discrete = _Base
    sys.modules["gym"] = gym
    sys.modules["gym.spaces"] = gym.spaces
    sys.modules["cv2"] = types.ModuleType("cv2")
    # the parent packages as namespaces: their __init__ files (env factories, simulators) are not executed
    for name in ("USTC_lab", "USTC_lab.env", "USTC_lab.env.gym_env"):
        if name not in sys.modules:
            pkg = types.ModuleType(name)
            pkg.__path__ = [os.path.join(REF, *name.split("."))]
            sys.modules[name] = pkg


def main():
    _install_stubs()
    RunningMeanStd = importlib.import_module("USTC_lab.env.gym_env.wrapper.warputils").RunningMeanStd
    rng = np.random.default_rng(28)
    rms = RunningMeanStd()
    out = {"batches": np.asarray(BATCHES, np.int64), "mean0": np.float64(rms.mean), "var0": np.float64(rms.var),
           "count0": np.float64(rms.count)}
    for i, n in enumerate(BATCHES):
        x = (OFFSET + SCALE * rng.standard_normal((n, D))).astype(np.float32).astype(np.float64)
        rms.update(x)
        out["x%d" % i] = x
        out["count%d" % (i + 1)] = np.float64(rms.count)
        out["mean%d" % (i + 1)] = np.asarray(rms.mean, np.float64)
        out["var%d" % (i + 1)] = np.asarray(rms.var, np.float64)
    np.savez(os.path.join(HERE, "f28_running_mean_std.npz"), **out)
    print("f28_running_mean_std.npz: count %g, mean %s, var %s" % (rms.count, rms.mean, rms.var))


if __name__ == "__main__":
    main()
