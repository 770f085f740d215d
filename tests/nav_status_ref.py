"""The rule book of the navigation info word and of the statistics kept from it (csrc/navenv.hip ddrl_op_nav_env_step_info,
csrc/navstat.hip, ddrl4nav_amd.agent.NavStatus).

The info word of one env step, int32:
  bit 0 done    bit 1 goal    bits 2-3 collision kind (0 none, 1 static = wall or obstacle, 2 pedestrian; static wins)
  bit 4 truncated    bit 5 close to a pedestrian (centres within CLOSE ticks after the move; never without pedestrians)
  bit 6 wall hit    bit 7 obstacle hit    bits 8-13 the decoded v (0..32)    bits 16-23 the decoded w + 64 (0..128)    others zero
It describes the step just played: NavInfoEnvRef reads it off the state after the move and before a finished env's new episode.

NavStatusRef is the per-env bookkeeping the reference's Status.update_nav_status keeps, in numpy float32 with its operation order, fed
by info words: arrive = goal bit, collision = the kind, all_down = the done bit, speeds = (v / 32, w / 64), bool_get_close_to_human =
bit 5, is_clean = 1.  Pinned to the reference's own class by tests/golden/f29_nav_status.npz."""
import numpy as np

import nav_env_ref as R

CLOSE = 512                                                             # 2 m
WINDOW = 100                                                            # Status.int_size
FAMILIES = ("", "_close_human", "_no_human")
ROWS = ("v_speeds_sum", "v_speeds_episode", "w_speeds_sum", "w_speeds_episode", "steps_sum", "steps_episode")
RINGS = ("arrive_num", "coll_static_num", "coll_ped_num", "coll_robot_num", "trunc_num")
PER_ENV = tuple(row + family for family in FAMILIES for row in ROWS) + ("episode_num",) + RINGS
SUMMARY_KEYS = ("ReducedReachRateLogger", "ReducedStaticObsCollisionRateLogger", "ReducedPedCollisionRateLogger", "TruncationRate",
                "ReducedLinearVelocityEpisodeLogger", "ReducedAngularVelocityEpisodeLogger",
                "ReducedCloseHumanLinearVelocityEpisodeLogger", "ReducedCloseHumanAngularVelocityEpisodeLogger",
                "ReducedOpenAreaLinearVelocityEpisodeLogger", "ReducedOpenAreaAngularVelocityEpisodeLogger", "ReducedStepsEpisodeLogger")
RATE_KEYS, SPEED_KEYS = SUMMARY_KEYS[:4], SUMMARY_KEYS[4:10]


def pack_info(done, goal, kind, trunc, close, wall, obstacle, v, w):
    """Arrays (or scalars) of the fields -> int32 words; w is signed (-64..64)."""
    f = [np.asarray(x, np.int64) for x in (done, goal, kind, trunc, close, wall, obstacle, v, w)]
    word = f[0] | (f[1] << 1) | (f[2] << 2) | (f[3] << 4) | (f[4] << 5) | (f[5] << 6) | (f[6] << 7) | (f[7] << 8) | ((f[8] + 64) << 16)
    return word.astype(np.int32)


def unpack_info(words):
    w = np.asarray(words).astype(np.int64)
    return {"done": w & 1, "goal": (w >> 1) & 1, "collision": (w >> 2) & 3, "truncated": (w >> 4) & 1, "close": (w >> 5) & 1,
            "wall_hit": (w >> 6) & 1, "obstacle_hit": (w >> 7) & 1, "v": (w >> 8) & 63, "w": ((w >> 16) & 255) - 64}


class NavInfoEnvRef(R.NavEnvRef):
    """NavEnvRef that also tells what happened: after step(), ``info`` holds the info words, ``played`` the state after the move and
    before the new episode of a finished env, ``events`` what NavEnvRef keeps."""

    def __init__(self, *args, ranges=True, **kw):
        """ranges=False: the laser component of the observation is all zeros (no ray is cast: most of the model's time); the info word,
        the state and the other components do not depend on it."""
        super().__init__(*args, **kw)
        self.ranges = bool(ranges)
        self.info = np.zeros(self.N, np.int32)
        self.played = self.state.copy()
        self._stepping = False

    def lidar(self):
        return super().lidar() if self.ranges else np.zeros((self.N, R.BEAMS), np.int64)

    def _new_episode(self, m):
        if self._stepping:                                              # step() draws the new episodes last: the move is complete
            self.played = self.state.copy()
        super()._new_episode(m)

    def step(self, actions):
        self._stepping = True
        try:
            obs, reward, done = super().step(actions)
        finally:
            self._stepping = False
        s, ev = self.played.astype(np.int64), self.events
        v, w = R.decode_actions(actions)
        close = np.zeros(self.N, bool)
        for j in range(self.n_peds):
            dx, dy = s[:, R.X] - s[:, R.PED0 + 4 * j], s[:, R.Y] - s[:, R.PED0 + 4 * j + 1]
            close |= dx * dx + dy * dy <= CLOSE * CLOSE
        static = (ev["wall_hit"] | ev["obstacle_hit"]) != 0
        kind = np.where(static, 1, np.where(ev["ped_hit"] != 0, 2, 0))
        self.info = pack_info(done, ev["goal"], kind, ev["trunc"], close, ev["wall_hit"], ev["obstacle_hit"], v, w)
        return obs, reward, done


def play_info(model, steps, rng, **kw):
    """nav_env_ref.play on a NavInfoEnvRef, also collecting the info words and the played states: (counts, actions, first, trace, info
    int32 [steps, N], played int32 [steps, N, 64])."""
    infos, played = [], []
    step = model.step

    def recording(actions):
        out = step(actions)
        infos.append(model.info.copy())
        played.append(model.played.copy())
        return out

    model.step = recording
    try:
        counts, actions, first, trace = R.play(model, steps, rng, **kw)
    finally:
        del model.step
    return counts, actions, first, trace, np.stack(infos), np.stack(played)


class NavStatusRef:
    """The navigation part of the reference's Status for N envs, float32; every attribute carries the reference's name (PER_ENV), plus
    trunc_num, a fifth ring kept by the rule of the other four."""

    def __init__(self, n_envs):
        self.N = int(n_envs)
        for name in PER_ENV:
            setattr(self, name, np.zeros(self.N, np.float32))
        self.episode_num = np.zeros(self.N, np.int32)
        for name in RINGS:
            setattr(self, name, np.zeros((WINDOW, self.N), np.float32))

    def _roll(self, name, family, add, down):
        """sum += add; episode = episode * (1 - down) + sum * down; sum *= (1 - down) -- float32 throughout."""
        s, e = name + "_sum" + family, name + "_episode" + family
        total = (getattr(self, s) + add).astype(np.float32)
        setattr(self, e, (getattr(self, e) * (np.float32(1) - down) + total * down).astype(np.float32))
        setattr(self, s, (total * (np.float32(1) - down)).astype(np.float32))

    def step(self, words):
        """One env step: words int32 [N]."""
        f = unpack_info(words)
        env = np.arange(self.N)
        slot = self.episode_num % WINDOW                                # the running episode's slot: overwritten by every step
        self.arrive_num[slot, env] = f["goal"]
        for kind, ring in ((1, self.coll_static_num), (2, self.coll_ped_num), (3, self.coll_robot_num)):
            ring[slot, env] = f["collision"] == kind
        self.trunc_num[slot, env] = f["truncated"]
        self.episode_num += f["done"].astype(np.int32)                  # and only then does the index advance
        down, close = f["done"].astype(np.float32), f["close"].astype(np.float32)
        av = np.abs(f["v"].astype(np.float32) * np.float32(2.0 ** -5))
        aw = np.abs(f["w"].astype(np.float32) * np.float32(2.0 ** -6))
        one = np.ones(self.N, np.float32)
        for family, weight in (("", one), ("_close_human", close), ("_no_human", one - close)):
            self._roll("v_speeds", family, av * weight, down)
            self._roll("w_speeds", family, aw * weight, down)
            self._roll("steps", family, one * weight, down)

    def update(self, words):
        """words int32 [T, N]: T steps."""
        for row in np.asarray(words).reshape(-1, self.N):
            self.step(row)

    def per_env(self):
        return {name: getattr(self, name).copy() for name in PER_ENV}

    def partial(self):
        """float64 [22]: the (sum, count) pairs of SUMMARY_KEYS.  Rates: sum(ring) / clip(episode_num + 1, 1, 100), every env counts.
        Speed means: the float32 quotient episode / steps of the family, over the envs whose steps are > 0.  Steps: every env."""
        out = np.zeros(2 * len(SUMMARY_KEYS), np.float64)
        window = np.clip(self.episode_num + 1, 1, WINDOW)
        for k, ring in enumerate((self.arrive_num, self.coll_static_num, self.coll_ped_num, self.trunc_num)):
            out[2 * k:2 * k + 2] = np.sum(np.sum(ring, 0) / window), self.N
        k = 4
        for family in FAMILIES:
            steps = getattr(self, "steps_episode" + family)
            has = steps > 0
            for name in ("v_speeds_episode", "w_speeds_episode"):
                q = (getattr(self, name + family)[has] / steps[has]).astype(np.float32)
                out[2 * k:2 * k + 2] = np.sum(q.astype(np.float64)), has.sum()
                k += 1
        out[2 * k:2 * k + 2] = np.sum(self.steps_episode.astype(np.float64)), self.N
        return out

    @staticmethod
    def summarize(partial):
        p = np.asarray(partial, np.float64)
        return {key: (p[2 * k] / p[2 * k + 1] if p[2 * k + 1] > 0 else float("nan")) for k, key in enumerate(SUMMARY_KEYS)}

    def summary(self):
        return self.summarize(self.partial())
