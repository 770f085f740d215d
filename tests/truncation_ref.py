"""The rule book of partial-episode bootstrapping, numpy only: the terminal observation of a truncated episode
on top of tests/nav_env_ref.py and tests/fleet_env_ref.py, the filing of flagged rows into per-env pools (csrc/truncate.hip) and GAE with
the successor value of a truncated step taken from those pools (ddrl_gae_bootstrap), in fp32 with the operation order of
oracle/ddrl_oracle.py:gae and again in float64."""
import copy

import numpy as np

import nav_env_ref as R

TRUNC_BIT = 1 << 4                                                      # info bit 4 (tests/nav_status_ref.py)


class NavEnvFinalRef(R.NavEnvRef):
    """NavEnvRef that keeps what a truncated env saw at its end: _new_episode, when step() calls it, first takes observe() of the state
    after rule 6 -- V and W the action just played, DPREV the distance after the move.  After a step, ``final`` is that snapshot
    ([laser, vector, image] of all N envs) and ``truncated`` the envs whose rows count (events["trunc"])."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._stepping = False
        self.final = None
        self.truncated = np.zeros(self.N, bool)

    def _new_episode(self, m):
        if self._stepping:
            self.final = self.observe()
        super()._new_episode(m)

    def step(self, actions):
        self._stepping = True
        try:
            out = super().step(actions)
        finally:
            self._stepping = False
        self.truncated = self.events["trunc"] != 0
        return out


def fleet_final_obs(model):
    """After FleetEnvRef.step: (the observation of every row with every robot where it is after all moves and before any respawn --
    observe() of a copy of the model whose state is ``played`` --, the rows it counts for: events["trunc"])."""
    twin = copy.copy(model)
    twin.state = model.played.copy()
    return twin.observe(), model.events["trunc"] != 0


def file_rows_ref(info, srcs, dsts, count, mask=TRUNC_BIT):
    """ddrl_op_file_flagged_rows: info int32 [N]; srcs [N, ...] and dsts [S, N, ...] per part; count int32 [N].  dsts and count change
    in place; returns slot_out int32 [N]."""
    info = np.asarray(info)
    n, s = len(info), dsts[0].shape[0]
    slot = np.full(n, -1, np.int32)
    for i in range(n):
        if not int(info[i]) & mask:
            continue
        c = int(count[i])
        if 0 <= c < s:
            for src, dst in zip(srcs, dsts):
                dst[c, i] = src[i]
            slot[i] = c
        count[i] = c + 1
    return slot


def gae_bootstrap_ref(values, rewards, dones, slots, boot, gamma=0.99, landa=0.95, dtype=np.float32):
    """oracle gae() with one change: where slots[t, n] is in [0, S) the successor term (gamma * V_next) * (1 - d) is
    gamma * boot[slots[t, n], n] -- a select.  dtype float32: the oracle's operation order, operation for operation; float64: the same
    expression in double precision.  -> (adv [T, N], ret [T, N])."""
    values = np.asarray(values, dtype)
    rewards, boot = np.asarray(rewards, dtype), np.asarray(boot, dtype)
    slots = np.asarray(slots)
    T, N, S = values.shape[0] - 1, values.shape[1], boot.shape[0]
    cols = np.arange(N)[None, :]
    discounts = np.array([gamma], dtype=dtype).reshape(1, 1)
    g = np.zeros_like(values[0:1])
    next_v = values[T:T + 1]
    adv = np.empty((T, N), dtype)
    ret = np.empty((T, N), dtype)
    for t in reversed(range(T)):
        d = dones[t:t + 1]
        v = values[t:t + 1]
        k = slots[t:t + 1]
        named = (k >= 0) & (k < S)
        b = boot[np.where(named, k, 0), cols]
        g = g * (1 - d)
        succ = np.where(named, discounts * b, discounts * next_v * (1 - d))
        g = discounts * landa * g + (succ - v + rewards[t:t + 1])
        next_v = v
        ret[t] = (v + g)[0]
        adv[t] = g[0] * 1.0
    return adv, ret
