"""RunningNorm: the running mean / variance of a stream of float rows, kept and applied on the device.

The reference ships ``RunningMeanStd`` (USTC_lab/env/gym_env/wrapper/warputils.py:83-109: Chan's parallel update of count, mean and
population variance) and wires it in nowhere; a host-side wrapper around it would pull every observation of a device-resident rollout
back across PCIe.  Here the same update runs in csrc/runnorm.hip on per-column sums:

    update(x)   adds the rows of x to the PENDING sums (n, sum x_j, sum x_j^2 in double; additive over calls and over ranks)
    commit()    all-reduces the pending sums over the process group when there is one, then merges them into the state with the
                reference's update -- every rank merges the same sums and holds a bit-identical state
    freeze()    forms the affine pair (shift = mean, scale = 1 / sqrt(var + eps)) that apply() uses until the next freeze()
    apply(x)    clamp((x - shift) * scale, -clip, clip), in place when out is x

A fresh state is the reference constructor's (count 0, mean 0, var 1): its frozen affine is (0, 1 / sqrt(1 + eps)).  DESIGN.md section
6.6 has the semantics the rollouts build on this."""
import math

import numpy as np
import torch

from ddrl4nav_amd import dist, ops


def check_knobs(eps, clip):
    """(eps, clip) as floats; eps >= 0 and finite, clip > 0 (inf allowed): ValueError otherwise."""
    try:
        eps, clip = float(eps), float(clip)
    except (TypeError, ValueError):
        raise ValueError("eps and clip must be numbers, got %r and %r" % (eps, clip)) from None
    if not (eps >= 0.0 and math.isfinite(eps)):
        raise ValueError("eps must be a finite number >= 0, got %r" % eps)
    if not clip > 0.0:
        raise ValueError("clip must be > 0 (inf = no clip), got %r" % clip)
    return eps, clip


def obs_norm_flags(normalize_obs, n_components):
    """One bool per observation component from the normalize_obs knob of StateRollout: None / False = none, True = every component,
    else a sequence of n_components bools (ValueError on any other length)."""
    if normalize_obs is None or normalize_obs is False:
        return [False] * n_components
    if normalize_obs is True:
        return [True] * n_components
    try:
        flags = [bool(f) for f in normalize_obs]
    except TypeError:
        raise ValueError("normalize_obs: True or one bool per observation component, got %r" % (normalize_obs,)) from None
    if len(flags) != n_components:
        raise ValueError("normalize_obs has %d entries for %d observation components" % (len(flags), n_components))
    return flags


class RunningNorm:
    def __init__(self, shape, device, eps=1e-8, clip=10.0, center=True):
        self.eps, self.clip = check_knobs(eps, clip)
        self.center = bool(center)
        self.shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        self.d = int(math.prod(self.shape))
        if self.d < 1:
            raise ValueError("shape %r holds no feature" % (shape,))
        dev = torch.device(device)
        self.device = dev
        self.state = ops.running_state(self.d, dev)                                  # count, mean[d], var[d]
        self.sums = torch.zeros(1 + 2 * self.d, dtype=torch.float64, device=dev)     # the pending batch
        self.affine = torch.empty((2, self.d), dtype=torch.float32, device=dev)      # shift[d], scale[d], as frozen
        self._pending = False
        self._ws = None
        self.freeze()

    # ---- statistics ---------------------------------------------------------------------------------
    @property
    def count(self):
        return self.state[0]

    @property
    def mean(self):
        return self.state[1:1 + self.d].view(self.shape)

    @property
    def var(self):
        return self.state[1 + self.d:].view(self.shape)

    def update(self, x):
        """Adds the rows of x ([n, *shape]: contiguous fp32 on the device, or a 2-D view with a row stride) to the pending sums."""
        n, _ = ops._rows2d(x, self.d)
        need = ops.column_moments_ws_floats(n, self.d)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
        ops.column_moments(x, self.d, sums=self.sums, accumulate=self._pending, ws=self._ws)
        self._pending = True

    def commit(self, group=None):
        """Merges the pending sums into the state, after one SUM all-reduce of them when a process group is initialised (every rank
        has to call it then, with or without pending rows of its own)."""
        if not self._pending:
            self.sums.zero_()
        dist.allreduce_flat(self.sums, group)
        ops.running_merge(self.sums, self.state)
        self._pending = False

    def freeze(self):
        ops.running_affine(self.state, self.eps, self.center, affine=self.affine)
        return self.affine

    def apply(self, x, out=None):
        """Normalises the rows of x with the frozen affine into `out` (x itself: in place; None: a new tensor).  Returns out."""
        return ops.normalize_columns(x, self.affine, self.clip, out=out)

    # ---- checkpoints ----------------------------------------------------------------------------------
    def state_dict(self):
        s = self.state.cpu()
        return {"count": s[0].clone(), "mean": s[1:1 + self.d].reshape(self.shape).clone(),
                "var": s[1 + self.d:].reshape(self.shape).clone(), "eps": self.eps, "clip": self.clip, "center": self.center}

    def load_state_dict(self, sd):
        """Takes count / mean / var and the three knobs, drops whatever is pending, and freezes."""
        mean = torch.as_tensor(sd["mean"], dtype=torch.float64).reshape(-1)
        var = torch.as_tensor(sd["var"], dtype=torch.float64).reshape(-1)
        if mean.numel() != self.d or var.numel() != self.d:
            raise ValueError("state of %d features loaded into a RunningNorm of %d" % (mean.numel(), self.d))
        self.eps, self.clip = check_knobs(sd["eps"], sd["clip"])
        self.center = bool(sd["center"])
        count = torch.as_tensor(sd["count"], dtype=torch.float64).reshape(1)
        self.state.copy_(torch.cat([count, mean, var]))
        self._pending = False
        self.freeze()


class ReturnNorm:
    """Return-based reward scaling of a rollout's finish(): the running variance of the discounted return g_t = gamma * g_{t-1} + r_t
    (zeroed behind a done; the carry [N] persists between rollouts) scales the rewards that GAE reads, rewards_norm = clamp(r /
    sqrt(var + eps), -clip, clip): no mean is subtracted.  The statistics are updated ONCE per rollout, with all of its T * N returns,
    BEFORE that rollout's own rewards are scaled -- per-step wrappers update after every env step."""

    def __init__(self, n_envs, horizon, gamma, device, eps=1e-8, clip=10.0):
        self.N, self.T = int(n_envs), int(horizon)
        self.gamma = float(np.float32(gamma))
        self.norm = RunningNorm(1, device, eps=eps, clip=clip, center=False)
        dev = self.norm.device
        self.carry = torch.zeros(self.N, dtype=torch.float32, device=dev)
        self.trace = torch.empty((self.T, self.N), dtype=torch.float32, device=dev)
        self.rewards_norm = torch.zeros((self.T, self.N), dtype=torch.float32, device=dev)

    def scale(self, rewards, dones):
        """rewards / dones [T, N] of the finished rollout -> rewards_norm [T, N]; the raw rewards are left as they are."""
        ops.discounted_returns(rewards, dones, self.gamma, self.carry, trace=self.trace)
        self.norm.update(self.trace.view(self.T * self.N, 1))
        self.norm.commit()
        self.norm.freeze()
        return self.norm.apply(rewards, out=self.rewards_norm)

    def state_dict(self):
        return {"norm": self.norm.state_dict(), "carry": self.carry.cpu()}

    def load_state_dict(self, sd):
        self.norm.load_state_dict(sd["norm"])
        self.carry.copy_(torch.as_tensor(sd["carry"], dtype=torch.float32).reshape(self.N))
