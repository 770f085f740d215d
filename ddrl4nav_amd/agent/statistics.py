"""EpisodeReturns and NavStatus: the reward and the navigation bookkeeping of the reference's ``Status`` (USTC_lab/agent/statistics.py:118-123,
``update_reward_status``) for a device-resident rollout.

The reference updates two per-env float32 vectors after every env step on the host:
    rewards_sum += rewards
    rewards_episode = rewards_episode * (1 - dones) + rewards_sum * dones     # the latest finished episode's return
    rewards_sum *= (1 - dones)
Here the rewards and dones of a whole rollout already sit in the experience pool ([T, N], agent/rollout.py), so the same
recurrence runs once per rollout in one small kernel (ddrl_episode_returns: one lane per env, the reference's operation
order, fp32) and the two vectors stay on the GPU between rollouts.  Pinned by golden F6 (the reference's own Status run).

NavStatus is the rest of Status for the device navigation env (statistics.py:66-116 ``update_nav_status``, 232-254 ``group_logger``):
reach, collision and truncation rates over the latest 100 episodes per env, steps and mean speeds per episode, fed by the info words
the env emits (ddrl_op_nav_env_step_info) and kept on the GPU (csrc/navstat.hip).  Pinned by golden F29."""
import math
from ctypes import c_void_p

import torch

from ddrl4nav_amd import _lib, ops
from ddrl4nav_amd._lib import check


class EpisodeReturns:
    def __init__(self, n_envs, device):
        self.lib = _lib.load()
        self.N = int(n_envs)
        dev = torch.device(device)
        self.rewards_sum = torch.zeros(self.N, dtype=torch.float32, device=dev)      # Status.rewards_sum
        self.rewards_episode = torch.zeros(self.N, dtype=torch.float32, device=dev)  # Status.rewards_episode
        self.episodes_finished = torch.zeros(self.N, dtype=torch.int32, device=dev)

    def update(self, rewards, dones, trace=None):
        """rewards f32 [T, N], dones u8 [T, N] (device, contiguous): T calls of update_reward_status in one launch.
        `trace` f32 [T, N] (optional) receives rewards_episode after every step."""
        T, N = rewards.shape
        if N != self.N or tuple(dones.shape) != (T, N):
            raise ValueError("rewards %s / dones %s do not match %d envs" % (tuple(rewards.shape), tuple(dones.shape), self.N))
        if rewards.dtype != torch.float32 or dones.dtype != torch.uint8 or not rewards.is_cuda:
            raise TypeError("rewards must be float32 and dones uint8 device tensors")
        if not (rewards.is_contiguous() and dones.is_contiguous()):
            raise ValueError("rewards / dones must be contiguous")
        if trace is not None and (tuple(trace.shape) != (T, N) or trace.dtype != torch.float32 or not trace.is_contiguous()):
            raise ValueError("trace must be a contiguous float32 [T, N] tensor")
        p = lambda t: c_void_p(0) if t is None else c_void_p(t.data_ptr())
        check(self.lib.ddrl_episode_returns(p(rewards), p(dones), T, N, p(self.rewards_sum), p(self.rewards_episode), p(trace),
                                            p(self.episodes_finished), c_void_p(torch.cuda.current_stream().cuda_stream)))
        return self.rewards_episode

    def mean_return(self):
        """Mean of the latest finished episode's return over the envs that have finished one (host float; synchronises)."""
        done = self.episodes_finished > 0
        k = int(done.sum().item())
        return float(self.rewards_episode[done].mean().item()) if k else float("nan")


_NAV_FAMILIES = ("", "_close_human", "_no_human")
_NAV_ROWS = ("v_speeds_sum", "v_speeds_episode", "w_speeds_sum", "w_speeds_episode", "steps_sum", "steps_episode")
_NAV_RINGS = ("arrive_num", "coll_static_num", "coll_ped_num", "coll_robot_num", "trunc_num")
# the (sum, count) pairs of ddrl_op_nav_status_reduce, in order
NAV_SUMMARY_KEYS = ("ReducedReachRateLogger", "ReducedStaticObsCollisionRateLogger", "ReducedPedCollisionRateLogger", "TruncationRate",
                    "ReducedLinearVelocityEpisodeLogger", "ReducedAngularVelocityEpisodeLogger",
                    "ReducedCloseHumanLinearVelocityEpisodeLogger", "ReducedCloseHumanAngularVelocityEpisodeLogger",
                    "ReducedOpenAreaLinearVelocityEpisodeLogger", "ReducedOpenAreaAngularVelocityEpisodeLogger",
                    "ReducedStepsEpisodeLogger")


class NavStatus:
    """Status.update_nav_status for N device envs.  The per-env state carries the reference's attribute names (v_speeds_sum,
    w_speeds_episode_close_human, steps_episode_no_human, episode_num, arrive_num [100, N], ...): views of the three buffers the
    kernels own -- ``sums`` fp32 [18, N], ``episode_num`` int32 [N], ``rings`` fp32 [5, 100, N].  ``trunc_num`` is a fifth ring kept by the
    ring rule of the other four: whether the episode ended by the time limit.  coll_robot_num counts collision kind 3, another robot: only
    a FleetNavEnv (env/fleet_nav_env.py, one status row per robot) emits it; other_robot_collision_rate() is its rate."""

    def __init__(self, n_envs, device):
        self.N = int(n_envs)
        if self.N < 1:
            raise ValueError("n_envs must be at least 1, got %d" % self.N)
        dev = torch.device(device)
        self.device = dev
        self.sums = torch.zeros((ops.NAV_STATUS_ROWS, self.N), dtype=torch.float32, device=dev)
        self.episode_num = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self.rings = torch.zeros((ops.NAV_STATUS_RINGS, ops.NAV_STATUS_WINDOW, self.N), dtype=torch.float32, device=dev)
        self._summary = torch.zeros(ops.NAV_STATUS_SUMMARY, dtype=torch.float64, device=dev)
        for f, family in enumerate(_NAV_FAMILIES):
            for k, row in enumerate(_NAV_ROWS):
                setattr(self, row + family, self.sums[f * len(_NAV_ROWS) + k])
        for g, ring in enumerate(_NAV_RINGS):
            setattr(self, ring, self.rings[g])

    def named_tensors(self):
        """{the reference's attribute name: its tensor (a view)} of every per-env quantity."""
        names = [row + family for family in _NAV_FAMILIES for row in _NAV_ROWS] + ["episode_num"] + list(_NAV_RINGS)
        return {k: getattr(self, k) for k in names}

    def update(self, info):
        """info int32 [T, N] (device, contiguous; the rows of a StateRollout's info pool): T calls of update_nav_status in one launch."""
        if info.dim() != 2 or info.shape[1] != self.N:
            raise ValueError("info %s does not match %d envs" % (tuple(info.shape), self.N))
        if info.dtype != torch.int32 or not info.is_cuda:
            raise TypeError("info must be an int32 device tensor")
        if not info.is_contiguous():
            raise ValueError("info must be contiguous")
        ops.nav_status_update(info, self.sums, self.episode_num, self.rings)

    def partial(self):
        """This rank's (sum, count) pairs: float64 [22] on the device (a buffer the status owns; asynchronous).  Partials of several
        ranks combine by adding."""
        return ops.nav_status_reduce(self.sums, self.episode_num, self.rings, self._summary)

    @staticmethod
    def combine(partials):
        """Host only: the sum of (sum, count) partials (sequences of 22 numbers, e.g. one per rank), a list of 22 floats."""
        rows = [[float(x) for x in (p.tolist() if hasattr(p, "tolist") else p)] for p in partials]
        if not rows or any(len(r) != ops.NAV_STATUS_SUMMARY for r in rows):
            raise ValueError("combine needs at least one partial of %d numbers" % ops.NAV_STATUS_SUMMARY)
        return [math.fsum(r[k] for r in rows) for k in range(ops.NAV_STATUS_SUMMARY)]

    def summary(self, partials=None):
        """{the reference's group_logger key: mean over the envs} plus TruncationRate, from host partials (e.g. gathered from every
        rank) or, by default, from this status: one device-to-host copy of 22 doubles, which synchronises.  A speed mean counts only the
        envs whose latest finished episode has steps of that kind; nan when there is none (EpisodeReturns.mean_return's convention)."""
        total = self.combine([self.partial().cpu()] if partials is None else partials)
        return {k: (total[2 * i] / total[2 * i + 1] if total[2 * i + 1] > 0 else float("nan")) for i, k in enumerate(NAV_SUMMARY_KEYS)}

    def other_robot_collision_rate(self):
        """ReducedOtherRobotCollisionRateLogger: the mean over the rows of sum(coll_robot_num, 0) / clip(episode_num + 1, 1, 100), the rule
        of the other collision rates of partial(); float64 on the device, returned as a host float (one scalar copy, which synchronises).
        Not one of summary()'s keys."""
        window = torch.clamp(self.episode_num + 1, 1, ops.NAV_STATUS_WINDOW).to(torch.float64)
        return float((self.coll_robot_num.to(torch.float64).sum(0) / window).mean().item())

    def state_dict(self):
        return {"sums": self.sums.cpu(), "episode_num": self.episode_num.cpu(), "rings": self.rings.cpu()}

    def load_state_dict(self, sd):
        for k in ("sums", "episode_num", "rings"):
            mine, t = getattr(self, k), torch.as_tensor(sd[k])
            if t.dtype != mine.dtype or tuple(t.shape) != tuple(mine.shape):
                raise ValueError("%s must be %s %s, got %s %s" % (k, mine.dtype, tuple(mine.shape), t.dtype, tuple(t.shape)))
        for k in ("sums", "episode_num", "rings"):
            getattr(self, k).copy_(torch.as_tensor(sd[k]))
