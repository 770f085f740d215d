"""The specification of the pedestrian model "avoid" (csrc/navcore.h nav_walk_peds_avoid): pedestrians that give
way to robots and to each other, as rule 1 of both navigation envs.  numpy int64 only, like tests/nav_env_ref.py and
tests/fleet_env_ref.py, whose units, tables, draws and every other rule this file takes over unchanged.  This file IS the rule book of
rule 1 under "avoid"; the kernels follow it.

Pedestrians walk in index order, so pedestrian k < j has already moved when j looks at it and k > j has not; the robots are where they
were before this step's moves (rule 1 precedes rule 2).  For pedestrian j at p with heading hp and speed sp:

  candidate of rank r   h_r = (hp + OFFSETS[r]) mod 3840, c_r = p + ((sp COS[h_r]) >> 14, (sp SIN[h_r]) >> 14)
  static refusal of c   rule 1 of "walk", word for word: |c|^2 > (2560 - 77)^2, or |c - ob|^2 < (77 + r_ob)^2 for an obstacle in use
  agent block of c      for any other pedestrian in use or any robot in use at q: |c - q|^2 < KEEP^2 and |c - q|^2 < |p - q|^2 (a step
                        that moves away from an intruder is never blocked)
  choice                c_0 statically refused: nothing moves and one draw sets the heading, exactly as under "walk" (pedestrians bounce
                        off walls and obstacles, they do not slide along them).  Otherwise the lowest rank whose candidate is neither
                        statically refused nor agent-blocked wins: p = c_r, heading = h_r (the turn persists), no draw.  No rank wins:
                        the position stays and one draw sets the heading to draw % 3840.  ped_turn counts every draw.

Every product fits 32 bits (|coordinate| <= 2560 + 24).  Two invariants follow (tests/test_ped_avoid_cpu.py): pedestrians that are
KEEP apart stay KEEP apart, and the distance between a pedestrian and a robot drops below KEEP only through the robot's own move."""
import copy

import numpy as np

import fleet_env_ref as F
import nav_env_ref as R
from nav_env_ref import ARENA_R, BONUS, COS, GOAL_TOL, HEADINGS, PED_R, Q, ROBOT_R, SIN, decode_actions, isqrt
from nav_status_ref import CLOSE, pack_info

KEEP = 192                                                              # one personal distance, centre to centre: 0.75 m
D = 320                                                                 # 30 degrees in heading steps
OFFSETS = np.array([0, D, -D, 2 * D, -2 * D, 3 * D, -3 * D], np.int64)  # in preference order: ranks 0..6
RANKS = len(OFFSETS)
MODELS = ("walk", "avoid")
BRANCHES = tuple("rank%d" % r for r in range(RANKS)) + ("static", "blocked")


def new_counts():
    return {k: 0 for k in BRANCHES}


def walk_avoid(obstacles, peds, robots, draw, counts=None, taken=None):
    """Rule 1 under "avoid" for M arenas at once.  obstacles = (x, y, r) int64 [M, n_obstacles] each; peds int64 [M, n_peds, 4] (x, y,
    heading, speed), moved IN PLACE; robots = (x, y) int64 [M, n_robots] each, where they stand before their moves; draw(mask [M]) -> one
    hash per arena, int64 [M], the event counter of the masked arenas going up (NavEnvRef._draw).  counts: a dict of BRANCHES that
    receives how often each branch was taken; taken: int64 [M, n_peds] that receives the index into BRANCHES of every pedestrian's branch.
    -> ped_turn int64 [M]: the draws of each arena."""
    ox, oy, orad = obstacles
    rx, ry = robots
    M, n_peds = peds.shape[0], peds.shape[1]
    turns = np.zeros(M, np.int64)
    for j in range(n_peds):
        px, py, hp, sp = (peds[:, j, i] for i in range(4))
        h = np.mod(hp[:, None] + OFFSETS[None, :], HEADINGS)            # [M, 7]
        cx, cy = px[:, None] + ((sp[:, None] * COS[h]) >> Q), py[:, None] + ((sp[:, None] * SIN[h]) >> Q)
        static = cx * cx + cy * cy > (ARENA_R - PED_R) ** 2
        if ox.shape[1]:
            static |= (((cx[:, :, None] - ox[:, None, :]) ** 2 + (cy[:, :, None] - oy[:, None, :]) ** 2)
                       < (PED_R + orad[:, None, :]) ** 2).any(axis=2)
        others = [k for k in range(n_peds) if k != j]
        qx = np.concatenate([peds[:, others, 0], rx], axis=1)           # [M, A]: the agents j gives way to, where they are now
        qy = np.concatenate([peds[:, others, 1], ry], axis=1)
        near = (cx[:, :, None] - qx[:, None, :]) ** 2 + (cy[:, :, None] - qy[:, None, :]) ** 2
        now = ((px[:, None] - qx) ** 2 + (py[:, None] - qy) ** 2)[:, None, :]
        blocked = ((near < KEEP * KEEP) & (near < now)).any(axis=2)
        free = ~static & ~blocked
        bounce = static[:, 0]
        none = ~bounce & ~free.any(axis=1)
        won = ~bounce & ~none
        rank = free.argmax(axis=1)                                      # the lowest free rank
        rows = np.arange(M)
        turn = bounce | none
        hd = draw(turn)
        peds[:, j, 0] = np.where(won, cx[rows, rank], px)
        peds[:, j, 1] = np.where(won, cy[rows, rank], py)
        peds[:, j, 2] = np.where(won, h[rows, rank], np.where(turn, hd % HEADINGS, hp))
        turns += turn
        if taken is not None:
            taken[:, j] = np.where(bounce, RANKS, np.where(none, RANKS + 1, rank))
        if counts is not None:
            for r in range(RANKS):
                counts["rank%d" % r] += int((won & (rank == r)).sum())
            counts["static"] += int(bounce.sum())
            counts["blocked"] += int(none.sum())
    return turns


def walk_plain(obstacles, peds, draw):
    """Rule 1 under "walk" (nav_env_ref.NavEnvRef.step, fleet_env_ref.FleetEnvRef.step), in walk_avoid's terms."""
    ox, oy, orad = obstacles
    turns = np.zeros(peds.shape[0], np.int64)
    for j in range(peds.shape[1]):
        px, py, hp, sp = (peds[:, j, i] for i in range(4))
        cx, cy = px + ((sp * COS[hp]) >> Q), py + ((sp * SIN[hp]) >> Q)
        refused = cx * cx + cy * cy > (ARENA_R - PED_R) ** 2
        if ox.shape[1]:
            refused |= (((cx[:, None] - ox) ** 2 + (cy[:, None] - oy) ** 2) < (PED_R + orad) ** 2).any(axis=1)
        h = draw(refused)
        peds[:, j, 0], peds[:, j, 1] = np.where(refused, px, cx), np.where(refused, py, cy)
        peds[:, j, 2] = np.where(refused, h % HEADINGS, hp)
        turns += refused
    return turns


def _check_model(ped_model):
    if ped_model not in MODELS:
        raise ValueError("ped_model must be one of %r, got %r" % (MODELS, ped_model))
    return ped_model


def min_ped_distance2(peds_xy):
    """The smallest squared centre distance between two pedestrians of int [M, n_peds, >= 2] (a large number below two pedestrians)."""
    p = np.asarray(peds_xy).astype(np.int64)
    n = p.shape[1]
    best = np.int64(1) << 40
    for a in range(n):
        for b in range(a + 1, n):
            best = min(best, int(((p[:, a, 0] - p[:, b, 0]) ** 2 + (p[:, a, 1] - p[:, b, 1]) ** 2).min()))
    return int(best)


class NavEnvPedRef(R.NavEnvRef):
    """NavEnvRef with a choice of rule 1: ped_model "walk" is NavEnvRef (step() is re-spelled, because NavEnvRef inlines its walk;
    tests/test_ped_avoid_cpu.py anchors the two bit for bit), "avoid" is walk_avoid.  Also what tests/nav_status_ref.py's and
    tests/truncation_ref.py's models keep: after step(), ``info`` holds the info words, ``played`` the state after the move and before
    the new episode of a finished env, and final_obs() renders the terminal observation of the truncated envs.  ``branches`` counts the
    branches of walk_avoid over the model's life."""

    def __init__(self, *args, ped_model="walk", ranges=True, **kw):
        super().__init__(*args, **kw)
        self.ped_model, self.ranges = _check_model(ped_model), bool(ranges)
        self.info = np.zeros(self.N, np.int32)
        self.played = self.state.copy()
        self.branches = new_counts()

    def lidar(self):
        return super().lidar() if self.ranges else np.zeros((self.N, R.BEAMS), np.int64)

    def _walk(self, robots):
        s = self.state
        peds = s[:, R.PED0:R.PED0 + 4 * self.n_peds].astype(np.int64).reshape(self.N, self.n_peds, 4)
        if self.ped_model == "avoid":
            turns = walk_avoid(self._obstacles(), peds, robots, self._draw, self.branches)
        else:
            turns = walk_plain(self._obstacles(), peds, self._draw)
        s[:, R.PED0:R.PED0 + 4 * self.n_peds] = peds.reshape(self.N, 4 * self.n_peds).astype(np.int32)
        return turns

    def step(self, actions):
        self.sanitize()
        s = self.state
        every = np.ones(self.N, bool)
        ev = {name: np.zeros(self.N, np.int64) for name in R.EVENT_NAMES}
        v, w = decode_actions(actions)
        ox, oy, orad = self._obstacles()
        # 1. the pedestrians: the robot stands where the last step left it
        ev["ped_turn"] = self._walk((s[:, R.X:R.X + 1].astype(np.int64), s[:, R.Y:R.Y + 1].astype(np.int64)))
        # 2. the robot  3. distance and reward units  4. collision  5. goal  6. truncation: NavEnvRef.step, line for line
        h = np.mod(s[:, R.H].astype(np.int64) + w, HEADINGS)
        x = s[:, R.X].astype(np.int64) + ((v * COS[h]) >> Q)
        y = s[:, R.Y].astype(np.int64) + ((v * SIN[h]) >> Q)
        for col, val in ((R.X, x), (R.Y, y), (R.H, h), (R.V, v), (R.W, w)):
            self._set(col, every, val)
        s[:, R.STEPS] = (s[:, R.STEPS].astype(np.uint32) + np.uint32(1)).astype(np.int32)
        d = isqrt((s[:, R.GX].astype(np.int64) - x) ** 2 + (s[:, R.GY].astype(np.int64) - y) ** 2)
        units = 2 * (s[:, R.DPREV].astype(np.int64) - d)
        self._set(R.DPREV, every, d)
        wall = x * x + y * y > (ARENA_R - ROBOT_R) ** 2
        hit_o = (((x[:, None] - ox) ** 2 + (y[:, None] - oy) ** 2) < (ROBOT_R + orad) ** 2).any(axis=1)
        px, py, _, _ = self._peds()
        dp = (x[:, None] - px) ** 2 + (y[:, None] - py) ** 2
        hit_p, close = (dp < (ROBOT_R + PED_R) ** 2).any(axis=1), (dp <= CLOSE * CLOSE).any(axis=1)
        collision = wall | hit_o | hit_p
        goal = ~collision & (d <= GOAL_TOL)
        trunc = ~collision & ~goal & (s[:, R.STEPS] >= self.max_steps)
        units = units - BONUS * collision + BONUS * goal
        ev["wall_hit"], ev["obstacle_hit"], ev["ped_hit"], ev["goal"], ev["trunc"] = (e.astype(np.int64) for e in (wall, hit_o, hit_p, goal, trunc))
        done = collision | goal | trunc
        kind = np.where(wall | hit_o, 1, np.where(hit_p, 2, 0))
        self.info = pack_info(done, goal, kind, trunc, close, wall, hit_o, v, w)
        reward = (units.astype(np.float32) * np.float32(2.0 ** -8)).astype(np.float32)
        self.played = self.state.copy()
        self._new_episode(done)
        self.events = ev
        return self.observe(), reward, done.astype(np.uint8)

    def final_obs(self):
        """After step(): (the observation of every env in the state its step ended in, the envs it counts for: events["trunc"])."""
        twin = copy.copy(self)
        twin.state = self.played.copy()
        return twin.observe(), self.events["trunc"] != 0


class FleetEnvPedRef(F.FleetEnvRef):
    """FleetEnvRef with a choice of rule 1, as NavEnvPedRef: "walk" is FleetEnvRef (step() re-spelled and anchored), "avoid" is
    walk_avoid with every robot in use, where it stands before this step's moves."""

    def __init__(self, *args, ped_model="walk", **kw):
        super().__init__(*args, **kw)
        self.ped_model = _check_model(ped_model)
        self.branches = new_counts()

    def step(self, actions):
        self.sanitize()
        s, nw, Rn = self.state, self.n_worlds, self.R
        ev = {k: np.zeros(nw if k in F.WORLD_EVENTS else self.N, np.int64) for k in F.EVENT_NAMES}
        v, w = (a.reshape(nw, Rn) for a in decode_actions(actions))
        ox, oy, orad = self._obstacles()
        # 1. the pedestrians
        rob = self._robots()
        peds = s[:, F.PED0:F.PED0 + 4 * self.n_peds].astype(np.int64).reshape(nw, self.n_peds, 4)
        if self.ped_model == "avoid":
            ev["ped_turn"] = walk_avoid((ox, oy, orad), peds, (rob[:, :, F.X], rob[:, :, F.Y]), self._draw, self.branches)
        else:
            ev["ped_turn"] = walk_plain((ox, oy, orad), peds, self._draw)
        s[:, F.PED0:F.PED0 + 4 * self.n_peds] = peds.reshape(nw, 4 * self.n_peds).astype(np.int32)
        # 2. to 6.: FleetEnvRef.step, line for line
        h = np.mod(rob[:, :, F.H] + w, HEADINGS)
        x = rob[:, :, F.X] + ((v * COS[h]) >> Q)
        y = rob[:, :, F.Y] + ((v * SIN[h]) >> Q)
        steps = (rob[:, :, F.STEPS].astype(np.uint32) + np.uint32(1)).astype(np.int32).astype(np.int64)
        d = isqrt((rob[:, :, F.GX] - x) ** 2 + (rob[:, :, F.GY] - y) ** 2)
        units = 2 * (rob[:, :, F.DPREV] - d)
        for f, val in ((F.X, x), (F.Y, y), (F.H, h), (F.V, v), (F.W, w), (F.STEPS, steps), (F.DPREV, d)):
            rob[:, :, f] = val
        self._put_robots(rob)
        wall = x * x + y * y > (ARENA_R - ROBOT_R) ** 2
        hit_o = (((x[:, :, None] - ox[:, None, :]) ** 2 + (y[:, :, None] - oy[:, None, :]) ** 2) < (ROBOT_R + orad[:, None, :]) ** 2).any(axis=2)
        px, py, _, _ = self._peds()
        dp = (x[:, :, None] - px[:, None, :]) ** 2 + (y[:, :, None] - py[:, None, :]) ** 2
        hit_p, close = (dp < (ROBOT_R + PED_R) ** 2).any(axis=2), (dp <= CLOSE * CLOSE).any(axis=2)
        dr = (x[:, :, None] - x[:, None, :]) ** 2 + (y[:, :, None] - y[:, None, :]) ** 2
        hit_r = ((dr < (2 * ROBOT_R) ** 2) & ~np.eye(Rn, dtype=bool)[None]).any(axis=2)
        static = wall | hit_o
        collision = static | hit_p | hit_r
        goal = ~collision & (d <= GOAL_TOL)
        trunc = ~collision & ~goal & (steps >= self.max_steps)
        units = units - BONUS * collision + BONUS * goal
        done = collision | goal | trunc
        kind = np.where(static, 1, np.where(hit_p, 2, np.where(hit_r, 3, 0)))
        flat = lambda a: np.asarray(a).reshape(self.N)
        self.info = pack_info(flat(done), flat(goal), flat(kind), flat(trunc), flat(close), flat(wall), flat(hit_o), flat(v), flat(w))
        for k, e in (("wall_hit", wall), ("obstacle_hit", hit_o), ("ped_hit", hit_p), ("robot_hit", hit_r), ("goal", goal), ("trunc", trunc)):
            ev[k] = flat(e).astype(np.int64)
        reward = (flat(units).astype(np.float32) * np.float32(2.0 ** -8)).astype(np.float32)
        self.played = self.state.copy()
        went = np.zeros((2, nw, Rn), np.int64)
        for r in range(Rn):
            went[0, :, r], went[1, :, r] = self._respawn(r, done[:, r])
        self.scan_cells = went.reshape(2, self.N)
        ev["start_advanced"], ev["goal_advanced"] = (self.scan_cells > 0).astype(np.int64)
        self.events = ev
        return self.observe(), reward, flat(done).astype(np.uint8)


# ---- crafted states ---------------------------------------------------------------------------------------------------------------------
def head_on_state():
    """int32 [1, 64]: the robot at the origin with a far goal, no obstacles, one pedestrian at (-400, 0) heading 0 at speed 16.  With
    n_obstacles = 0, n_peds = 1 and every action (0, 0): "walk" runs the pedestrian into the robot, "avoid" leads it around."""
    s = np.zeros((1, R.STATE_INTS), np.int32)
    s[0, R.GX], s[0, R.GY], s[0, R.DPREV] = 2000, 0, 2000
    s[0, R.PED0:R.PED0 + 4] = (-400, 0, 0, 16)
    return s


BRANCH_POPULATION = dict(n_obstacles=1, n_peds=5)
BRANCH_SEED, BRANCH_DRAWS = 5, 40000


def _branch_candidates():
    """int32 [BRANCH_DRAWS, 64], seeded: pedestrian 0 at the origin, heading 0, speed 16; pedestrians 1..4 and the robot scattered
    150..260 ticks around it (so some candidates of pedestrian 0 come within KEEP of them and nearer than now); the obstacle right ahead
    in every eighth state and far away in the others; the robot's goal far away."""
    rng = np.random.RandomState(BRANCH_SEED)
    m = BRANCH_DRAWS
    s = np.zeros((m, R.STATE_INTS), np.int32)
    rad, ang = rng.randint(150, 261, (m, 5)), rng.randint(0, HEADINGS, (m, 5))
    x, y = (rad * COS[ang]) >> Q, (rad * SIN[ang]) >> Q
    s[:, R.X], s[:, R.Y], s[:, R.H] = x[:, 4], y[:, 4], rng.randint(0, HEADINGS, m)
    s[:, R.GX], s[:, R.GY] = 0, 2400
    s[:, R.DPREV] = isqrt((s[:, R.GX].astype(np.int64) - x[:, 4]) ** 2 + (s[:, R.GY].astype(np.int64) - y[:, 4]) ** 2)
    ahead = np.arange(m) % 8 == 0
    s[:, R.OBS0], s[:, R.OBS0 + 1], s[:, R.OBS0 + 2] = np.where(ahead, 150, 0), np.where(ahead, 0, -2300), 100
    s[:, R.PED0:R.PED0 + 4] = (0, 0, 0, 16)
    for i in range(4):
        c = R.PED0 + 4 * (i + 1)
        s[:, c], s[:, c + 1], s[:, c + 2], s[:, c + 3] = x[:, i], y[:, i], rng.randint(0, HEADINGS, m), rng.randint(8, 25, m)
    return s


def first_ped_branch(state, n_obstacles=1, n_peds=5):
    """The branch pedestrian 0 of every state int32 [M, 64] (sanitised) takes under "avoid": an index into BRANCHES, int64 [M]."""
    s = np.asarray(state).astype(np.int64)
    m = len(s)
    peds = s[:, R.PED0:R.PED0 + 4 * n_peds].reshape(m, n_peds, 4).copy()
    obst = s[:, R.OBS0:R.OBS0 + 3 * n_obstacles].reshape(m, n_obstacles, 3)
    agents = (np.concatenate([peds[:, 1:, 0], s[:, R.X:R.X + 1]], axis=1), np.concatenate([peds[:, 1:, 1], s[:, R.Y:R.Y + 1]], axis=1))
    taken = np.zeros((m, 1), np.int64)
    walk_avoid((obst[:, :, 0], obst[:, :, 1], obst[:, :, 2]), peds[:, :1].copy(), agents, lambda mask: np.zeros(m, np.int64), taken=taken)
    return taken[:, 0]


def branch_states():
    """int32 [9, 64] for BRANCH_POPULATION: state k is the first of the seeded candidates in which pedestrian 0 takes branch BRANCHES[k]
    -- ranks 0..6 won, the static refusal of rank 0, every rank blocked.  Crafted states: they need not respect the spacing a reset
    gives."""
    cand = _branch_candidates()
    taken = first_ped_branch(cand, **BRANCH_POPULATION)
    out = np.zeros((len(BRANCHES), R.STATE_INTS), np.int32)
    for k in range(len(BRANCHES)):
        hits = np.nonzero(taken == k)[0]
        assert len(hits), "no seeded candidate takes branch %s" % BRANCHES[k]
        out[k] = cand[hits[0]]
    return out


# ---- tapes ------------------------------------------------------------------------------------------------------------------------------
def nav_coverage_run(ped_model, **over):
    """nav_env_ref.coverage_run on a NavEnvPedRef: -> (model, counts, actions, first, trace, info int32 [steps, N], played, final
    [(obs, rows)] per step)."""
    model = NavEnvPedRef(ped_model=ped_model, **dict(R.COVERAGE, **over))
    infos, played, finals = [], [], []
    step = model.step

    def recording(actions):
        out = step(actions)
        infos.append(model.info.copy())
        played.append(model.played.copy())
        finals.append(model.final_obs() if model.ranges and model.events["trunc"].any() else (None, model.events["trunc"] != 0))
        return out

    model.step = recording
    try:
        counts, actions, first, trace = R.play(model, R.COVERAGE_STEPS, np.random.RandomState(0))
    finally:
        del model.step
    return model, counts, actions, first, trace, np.stack(infos), np.stack(played), finals


def fleet_coverage_run(ped_model, steps=F.COVERAGE_STEPS, **over):
    """fleet_env_ref.coverage_run on a FleetEnvPedRef: -> (model, counts, actions, first, trace)."""
    model = FleetEnvPedRef(ped_model=ped_model, **dict(F.COVERAGE, **over))
    return (model,) + F.play(model, steps, np.random.RandomState(0))


def expert_tape(ped_model, n_envs, steps, seed, n_obstacles, n_peds, max_steps):
    """nav_expert_ref.expert_tape on a NavEnvPedRef without ranges.  -> (event totals, branch counts of walk_avoid)."""
    import nav_expert_ref as E
    m = NavEnvPedRef(n_envs, seed=seed, n_obstacles=n_obstacles, n_peds=n_peds, max_steps=max_steps, ped_model=ped_model, ranges=False)
    m.observe = lambda: None
    m.reset()
    totals = {k: 0 for k in E.EVENTS}
    for _ in range(steps):
        m.step(E.expert_labels(m.state, n_obstacles, n_peds))
        for k in E.EVENTS:
            totals[k] += int(m.events[k].sum())
    return totals, dict(m.branches)
