"""The specification of the scripted navigation expert (csrc/navexpert.hip, ddrl4nav_amd.env.NavExpert), as
tests/nav_env_ref.py is the env's: numpy int64 only, so the kernel's labels and played actions compare bit for bit.  This file IS the
rule book; the kernel follows it.

Input: the 64 state words of an env, sanitised as the step kernel sanitises them (NavEnvRef.sanitize), and the populations.

  candidates  c = 0..50: v = (32, 16, 4)[c // 17], w = -64 + 8 (c % 17)
  arc         k = 1..10: h = (h + w) mod 3840, x += (v COS[h]) >> 14, y += (v SIN[h]) >> 14 (the robot's own rules); pedestrian j is
              predicted at p_j + k ((speed COS[hp]) >> 14, (speed SIN[hp]) >> 14).  The arc is hit at step k if x^2 + y^2 >
              (2560 - 64 - 24)^2, or |pos - ob|^2 < (64 + 24 + r)^2 for an obstacle in use, or |pos - ped_k|^2 < (64 + 77 + 48)^2 for a
              pedestrian in use.  kc = the first hit step, 11 without one.  best = min over k < kc of isqrt(|goal - pos|^2), from 8191.
              The pose integrates to k = 10 whatever was hit.
  bearing     (ex, ey) = the goal in the robot frame at the final pose (>> 14 floors), dend = isqrt(|goal - pos|^2);
              bear = dend if ex <= 0 else min(|ey|, dend)
  choice      cost = (0 if best <= 77 else best + (bear >> 1)) + 4096 (11 - kc); key = 64 cost + c; the smallest key wins (< 2^22)
  label       (v / 32, w / 64) in fp32: both exact, and the env's decode returns v, w
  mixing      played[i] = label[i] if hash32(seed, global env index, step) < threshold else policy[i]; threshold =
              min(2^32 - 1, floor(beta 2^32)); the draw does not touch the env's event counter"""
import numpy as np

from device_env_ref import hash32
from nav_env_ref import (ARENA_R, COS, DPREV_MAX, GOAL_TOL, GX, GY, H, HEADINGS, OBS0, PED0, PED_R, Q, ROBOT_R, SIN, X, Y, NavEnvRef,
                         decode_actions, isqrt)

N_CANDIDATES, N_SPEEDS, N_TURNS = 51, 3, 17
SPEEDS = np.array([32, 16, 4], np.int64)
HORIZON = 10
MARGIN_STATIC, MARGIN_PED = 24, 48
NO_HIT = HORIZON + 1
HIT_COST = 4096
KEY_LIMIT = 1 << 22

BRANCHES = ("arc_wall", "arc_obstacle", "arc_ped", "arc_free", "arrives", "goal_behind", "key_tie")


def candidates():
    """(v, w) int64 [51] each."""
    c = np.arange(N_CANDIDATES, dtype=np.int64)
    return SPEEDS[c // N_TURNS], -64 + 8 * (c % N_TURNS)


def sanitized(state, n_obstacles, n_peds):
    """A sanitised int64 copy of state int32 [N, 64] (NavEnvRef.sanitize on a copy: the expert never writes the env)."""
    state = np.asarray(state, np.int32)
    m = NavEnvRef(state.shape[0], n_obstacles=n_obstacles, n_peds=n_peds)
    m.state = state.copy()
    m.sanitize()
    return m.state.astype(np.int64)


def expert_keys(state, n_obstacles, n_peds, counts=None):
    """key int64 [N, 51] of every candidate.  counts: a dict that receives how often each branch of BRANCHES was taken."""
    s = sanitized(state, n_obstacles, n_peds)
    n = s.shape[0]
    v, w = (a[None, :] for a in candidates())
    x = np.repeat(s[:, X, None], N_CANDIDATES, axis=1)
    y = np.repeat(s[:, Y, None], N_CANDIDATES, axis=1)
    h = np.repeat(s[:, H, None], N_CANDIDATES, axis=1)
    gx, gy = s[:, GX, None], s[:, GY, None]
    kc = np.full((n, N_CANDIDATES), NO_HIT, np.int64)
    best = np.full((n, N_CANDIDATES), DPREV_MAX, np.int64)
    first = {k: np.zeros((n, N_CANDIDATES), bool) for k in ("arc_wall", "arc_obstacle", "arc_ped")}
    for k in range(1, HORIZON + 1):
        h = np.mod(h + w, HEADINGS)
        x = x + ((v * COS[h]) >> Q)
        y = y + ((v * SIN[h]) >> Q)
        wall = x * x + y * y > (ARENA_R - ROBOT_R - MARGIN_STATIC) ** 2
        hit_o = np.zeros_like(wall)
        for o in range(n_obstacles):
            ox, oy, orad = (s[:, OBS0 + 3 * o + i, None] for i in range(3))
            hit_o |= (x - ox) ** 2 + (y - oy) ** 2 < (ROBOT_R + MARGIN_STATIC + orad) ** 2
        hit_p = np.zeros_like(wall)
        for j in range(n_peds):
            px, py, hp, sp = (s[:, PED0 + 4 * j + i, None] for i in range(4))
            qx, qy = px + k * ((sp * COS[hp]) >> Q), py + k * ((sp * SIN[hp]) >> Q)
            hit_p |= (x - qx) ** 2 + (y - qy) ** 2 < (ROBOT_R + PED_R + MARGIN_PED) ** 2
        new = (kc == NO_HIT) & (wall | hit_o | hit_p)
        for name, m in (("arc_wall", wall), ("arc_obstacle", hit_o), ("arc_ped", hit_p)):
            first[name] |= new & m
        kc = np.where(new, k, kc)
        d = isqrt((gx - x) ** 2 + (gy - y) ** 2)
        best = np.where(kc == NO_HIT, np.minimum(best, d), best)
    dx, dy = gx - x, gy - y
    ex, ey = (dx * COS[h] + dy * SIN[h]) >> Q, (-dx * SIN[h] + dy * COS[h]) >> Q
    dend = isqrt(dx * dx + dy * dy)
    bear = np.where(ex <= 0, dend, np.minimum(np.abs(ey), dend))
    cost = np.where(best <= GOAL_TOL, 0, best + (bear >> 1)) + HIT_COST * (NO_HIT - kc)
    key = 64 * cost + np.arange(N_CANDIDATES, dtype=np.int64)[None, :]
    if counts is not None:
        for name in first:
            counts[name] = counts.get(name, 0) + int(first[name].sum())
        counts["arc_free"] = counts.get("arc_free", 0) + int((kc == NO_HIT).sum())
        counts["arrives"] = counts.get("arrives", 0) + int((best <= GOAL_TOL).sum())
        counts["goal_behind"] = counts.get("goal_behind", 0) + int((ex <= 0).sum())
        lowest = cost.min(axis=1, keepdims=True)
        counts["key_tie"] = counts.get("key_tie", 0) + int(((cost == lowest).sum(axis=1) > 1).sum())
        counts["max_key"] = max(counts.get("max_key", 0), int(key.max()))
    return key


def expert_choice(state, n_obstacles, n_peds, counts=None):
    """(v, w) int64 [N] of the winning candidate."""
    c = expert_keys(state, n_obstacles, n_peds, counts).min(axis=1) & 63
    v, w = candidates()
    return v[c], w[c]


def expert_labels(state, n_obstacles, n_peds, counts=None):
    """float32 [N, 2]: (v / 32, w / 64), exact."""
    v, w = expert_choice(state, n_obstacles, n_peds, counts)
    return np.stack([v.astype(np.float32) * np.float32(2.0 ** -5), w.astype(np.float32) * np.float32(2.0 ** -6)], axis=1)


def beta_threshold(beta):
    """uint32 threshold of DAgger's beta: min(2^32 - 1, floor(beta 2^32)) for 0 <= beta <= 1."""
    beta = float(beta)
    if not 0.0 <= beta <= 1.0:
        raise ValueError("beta must be in [0, 1], got %r" % beta)
    return min(2 ** 32 - 1, int(np.floor(beta * 2.0 ** 32)))


def expert_mask(n, seed, env0, step, threshold):
    """bool [N]: the envs that play the expert's label at `step`."""
    genv = (np.arange(n, dtype=np.int64) + int(env0)).astype(np.uint32)
    draw = hash32(int(seed) & 0xFFFFFFFF, genv, np.full(n, int(step) & 0xFFFFFFFF, np.uint32))
    return draw.astype(np.int64) < int(threshold)


def mix(labels, policy, seed, env0, step, threshold):
    """played float32 [N, 2]: the label where the draw is below the threshold, the policy's action elsewhere (bits kept)."""
    labels, policy = np.asarray(labels, np.float32), np.asarray(policy, np.float32)
    return np.where(expert_mask(labels.shape[0], seed, env0, step, threshold)[:, None], labels, policy)


class NavEnvRefNoRender(NavEnvRef):
    """NavEnvRef whose step skips the render: the expert reads the state, and a tape of thousands of steps needs no lidar."""

    def observe(self):
        return None


EVENTS = ("goal", "obstacle_hit", "ped_hit", "wall_hit", "trunc")


def expert_tape(n_envs, steps, seed, n_obstacles, n_peds, max_steps, env0=0, counts=None, record=False):
    """Plays the expert on the rule book's env from a reset.  -> (event totals {name: count}, [(state before, label)] when record)."""
    m = NavEnvRefNoRender(n_envs, seed=seed, n_obstacles=n_obstacles, n_peds=n_peds, max_steps=max_steps, env0=env0)
    m.reset()
    totals, tape = {k: 0 for k in EVENTS}, []
    for _ in range(steps):
        a = expert_labels(m.state, n_obstacles, n_peds, counts)
        if record:
            tape.append((m.state.copy(), a))
        m.step(a)
        for k in EVENTS:
            totals[k] += int(m.events[k].sum())
    return totals, tape


def reach_rate(totals):
    """goals / finished episodes (1.0 when nothing finished)."""
    done = totals["goal"] + totals["obstacle_hit"] + totals["ped_hit"] + totals["wall_hit"] + totals["trunc"]
    return totals["goal"] / done if done else 1.0


def label_decodes(labels):
    """(v, w) the env decodes a float32 [N, 2] label to (nav_env_ref.decode_actions)."""
    return decode_actions(labels)


COVERAGE = dict(n_envs=8, steps=60, seed=7, n_obstacles=10, n_peds=5, max_steps=120)


def coverage_states():
    """The seeded states of the branch-coverage check, int32 [960, 64]: the 480 states the expert visits on the COVERAGE tape, and the
    same 480 with the robot moved onto a ring next to the wall (radius 2,250..2,490, seeded), where arcs leave the arena."""
    _, tape = expert_tape(record=True, **COVERAGE)
    inner = np.concatenate([s for s, _ in tape])
    rng = np.random.RandomState(11)
    outer = inner.copy()
    rad, ang = rng.randint(2250, 2491, len(outer)), rng.randint(0, HEADINGS, len(outer))
    outer[:, X] = (rad * COS[ang]) >> Q
    outer[:, Y] = (rad * SIN[ang]) >> Q
    return np.concatenate([inner, outer])
