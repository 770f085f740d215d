"""The specification of the device environments (csrc/denv.hip, ddrl4nav_amd/env): Pong and Catch on an 84 x 84
uint8 court, vectorised over N envs, in numpy with int32 / uint32 arithmetic only -- no floating point enters the dynamics, so the
kernels reproduce every state word, frame byte, reward and done bit for bit.  This file IS the rule book; the kernels follow it.

State: int32 [N][16] (STATE_INTS words per env)
  0 BX  ball left column        1 BY  ball top row            2 VX  ball x velocity      3 VY  ball y velocity
  4 PA  agent paddle (Pong: top row, Catch: left column)      5 PO  opponent paddle top row (Pong)
  6 SA  agent's points          7 SO  opponent's points       8 STEPS steps of the episode
  9 EVENTS hash draws so far (never reset by an episode's end: every serve of an env differs)      10..15 zero

Actions are float32 [N], as the acting kernels write them: k = int(a) % 3 is stay / negative direction / positive direction; an action
that is not finite, negative or >= n_actions is a NOOP (k = 0).  Envs reset themselves: on done the returned state and frame are the
first of the next episode."""
import numpy as np

STATE_INTS = 16
BX, BY, VX, VY, PA, PO, SA, SO, STEPS, EVENTS = range(10)
SIZE = 84
PLANE = SIZE * SIZE
BACKGROUND, OBJECT = 87, 236
PONG, CATCH = 0, 1
GAMES = {"pong": PONG, "catch": CATCH}

# Pong: paddles 2 x 10 (opponent columns 4..5, agent columns 78..79, top row 0..74), ball 2 x 2, vx = +-2, vy in -3..3
PONG_PADDLE_H, PONG_PADDLE_MAX = 10, SIZE - 10
PONG_OPP_X, PONG_AGENT_X = 4, 78
PONG_BALL, PONG_BALL_MAX = 2, SIZE - 2
PONG_AGENT_SPEED, PONG_OPP_SPEED, PONG_VX, PONG_VY_MAX = 3, 2, 2, 3
PONG_SERVE_X, PONG_PADDLE_START = 41, 37
PONG_HIT_AGENT_X, PONG_HIT_OPP_X = 76, 6          # where a returned ball is placed
# Catch: paddle 12 x 2 at rows 80..81 (left column 0..72), ball 4 x 4 falling 4 rows a step, drifting vx in -1..1
CATCH_PADDLE_W, CATCH_PADDLE_MAX, CATCH_PADDLE_Y, CATCH_PADDLE_H = 12, SIZE - 12, 80, 2
CATCH_BALL, CATCH_BALL_MAX, CATCH_FALL, CATCH_SPEED, CATCH_PADDLE_START = 4, SIZE - 4, 4, 4, 36

EVENT_NAMES = ("wall", "agent_hit", "opp_hit", "won", "lost", "score_done", "trunc_done")


def hash32(seed, env, counter):
    """The counter-based hash: uint32 words in, a uint32 out; no state beyond the counter."""
    with np.errstate(over="ignore"):
        x = (np.uint32(seed) ^ (np.asarray(env).astype(np.uint32) * np.uint32(0x9E3779B1))
             ^ (np.asarray(counter).astype(np.uint32) * np.uint32(0x85EBCA77)))
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x846CA68B)
        x = x ^ (x >> np.uint32(16))
    return x


def decode_actions(actions, n_actions):
    """float32 [N] -> k in {0, 1, 2}; hostile values are NOOPs."""
    a = np.asarray(actions, np.float32)
    ok = np.isfinite(a) & (a >= 0) & (a < np.float32(n_actions))
    return (np.where(ok, a, np.float32(0)).astype(np.int32) % 3).astype(np.int32)


class DeviceEnvRef:
    def __init__(self, game, n_envs, seed=0, n_actions=6, points=21, max_steps=10000, env0=0):
        self.game = GAMES[game] if isinstance(game, str) else int(game)
        assert self.game in (PONG, CATCH) and n_envs >= 1 and 2 <= n_actions <= 18 and points >= 1 and max_steps >= 1
        self.N, self.seed, self.n_actions, self.points, self.max_steps = int(n_envs), int(seed) & 0xFFFFFFFF, n_actions, points, max_steps
        self.genv = (np.arange(self.N, dtype=np.int64) + int(env0)).astype(np.uint32)
        self.state = np.zeros((self.N, STATE_INTS), np.int32)
        self.events = {k: np.zeros(self.N, bool) for k in EVENT_NAMES}   # what happened in the LAST step (the model's own bookkeeping)

    # ---- pieces -------------------------------------------------------------------------------------------------------------------------
    def _draw(self, m):
        """One hash per env of the mask `m`; the event counter of those envs advances."""
        s = self.state
        h = hash32(self.seed, self.genv, s[:, EVENTS].astype(np.uint32))
        s[:, EVENTS] = np.where(m, (s[:, EVENTS].astype(np.uint32) + np.uint32(1)).astype(np.int32), s[:, EVENTS])
        return h

    def _serve(self, m):
        """Pong: the ball re-serves from column 41; Catch: a new ball at the top."""
        s = self.state
        h = self._draw(m)
        if self.game == PONG:
            bx = np.full(self.N, PONG_SERVE_X, np.int32)
            by = ((h >> np.uint32(4)) % np.uint32(PONG_BALL_MAX + 1)).astype(np.int32)
            vx = np.where((h & np.uint32(1)) != 0, PONG_VX, -PONG_VX).astype(np.int32)
            vy = ((h >> np.uint32(1)) % np.uint32(2 * PONG_VY_MAX + 1)).astype(np.int32) - PONG_VY_MAX
        else:
            bx = (h % np.uint32(CATCH_BALL_MAX + 1)).astype(np.int32)
            by = np.zeros(self.N, np.int32)
            vx = ((h >> np.uint32(8)) % np.uint32(3)).astype(np.int32) - 1
            vy = np.full(self.N, CATCH_FALL, np.int32)
        for col, v in ((BX, bx), (BY, by), (VX, vx), (VY, vy)):
            s[:, col] = np.where(m, v, s[:, col])

    def _new_episode(self, m):
        s = self.state
        start = PONG_PADDLE_START if self.game == PONG else CATCH_PADDLE_START
        s[:, PA] = np.where(m, start, s[:, PA])
        s[:, PO] = np.where(m, PONG_PADDLE_START if self.game == PONG else 0, s[:, PO])
        for col in (SA, SO, STEPS):
            s[:, col] = np.where(m, 0, s[:, col])
        self._serve(m)

    def sanitize(self):
        """What the kernels do to the words they load, so that no state -- not even a corrupted one -- leaves the court: positions and
        velocities are clamped to their ranges (a no-op on every state the rules produce); the counters pass."""
        s = self.state
        if self.game == PONG:
            s[:, BX] = np.clip(s[:, BX], 0, PONG_BALL_MAX)
            s[:, BY] = np.clip(s[:, BY], 0, PONG_BALL_MAX)
            s[:, VX] = np.where(s[:, VX] > 0, PONG_VX, -PONG_VX)
            s[:, VY] = np.clip(s[:, VY], -PONG_VY_MAX, PONG_VY_MAX)
            s[:, PA] = np.clip(s[:, PA], 0, PONG_PADDLE_MAX)
            s[:, PO] = np.clip(s[:, PO], 0, PONG_PADDLE_MAX)
        else:
            s[:, BX] = np.clip(s[:, BX], 0, CATCH_BALL_MAX)
            s[:, BY] = np.clip(s[:, BY], 0, CATCH_BALL_MAX)
            s[:, VX] = np.clip(s[:, VX], -1, 1)
            s[:, VY] = CATCH_FALL
            s[:, PA] = np.clip(s[:, PA], 0, CATCH_PADDLE_MAX)
            s[:, PO] = 0
        s[:, 10:] = 0

    # ---- the public surface ---------------------------------------------------------------------------------------------------------------
    def reset(self, mask=None):
        """Every env, or those with a non-zero mask byte: all words zero (the event counter too), then a new episode.  Returns the frames."""
        m = np.ones(self.N, bool) if mask is None else (np.asarray(mask).reshape(self.N) != 0)
        self.state[m] = 0
        self._new_episode(m)
        return self.render()

    def step(self, actions):
        """-> (frame uint8 [N, 84, 84], reward float32 [N], done uint8 [N])."""
        self.sanitize()
        s = self.state
        k = decode_actions(actions, self.n_actions)
        move = np.where(k == 1, -1, np.where(k == 2, 1, 0)).astype(np.int32)
        ev = {name: np.zeros(self.N, bool) for name in EVENT_NAMES}
        reward = np.zeros(self.N, np.int32)
        if self.game == PONG:
            # 1. the agent's paddle  2. the opponent follows the ball's centre row (as it was before the ball moves), only while it approaches
            s[:, PA] = np.clip(s[:, PA] + move * PONG_AGENT_SPEED, 0, PONG_PADDLE_MAX)
            want = s[:, BY] + 1 - PONG_PADDLE_H // 2
            d = np.clip(want - s[:, PO], -PONG_OPP_SPEED, PONG_OPP_SPEED)
            s[:, PO] = np.where(s[:, VX] < 0, np.clip(s[:, PO] + d, 0, PONG_PADDLE_MAX), s[:, PO])
            # 3. the ball: rows reflect at 0 / 82, columns move
            y, vy = s[:, BY] + s[:, VY], s[:, VY].copy()
            low, high = y < 0, y > PONG_BALL_MAX
            y = np.where(low, -y, np.where(high, 2 * PONG_BALL_MAX - y, y))
            vy = np.where(low | high, -vy, vy)
            ev["wall"] = low | high
            x = s[:, BX] + s[:, VX]
            # 4. at a paddle's column: a hit returns the ball, a miss is a point and a serve
            at_agent, at_opp = x >= PONG_AGENT_X - 1, x <= PONG_OPP_X + 1
            pad = np.where(at_agent, s[:, PA], s[:, PO])
            overlap = (y + PONG_BALL - 1 >= pad) & (y <= pad + PONG_PADDLE_H - 1)
            hit = (at_agent | at_opp) & overlap
            off = y + 1 - (pad + PONG_PADDLE_H // 2)
            spin = np.clip((off - (off & 1)) // 2, -PONG_VY_MAX, PONG_VY_MAX)     # floor(off / 2)
            x = np.where(hit, np.where(at_agent, PONG_HIT_AGENT_X, PONG_HIT_OPP_X), x)
            vx = np.where(hit, -s[:, VX], s[:, VX])
            vy = np.where(hit, spin, vy)
            s[:, BX], s[:, BY], s[:, VX], s[:, VY] = x, y, vx, vy
            won, lost = at_opp & ~overlap, at_agent & ~overlap
            ev["agent_hit"], ev["opp_hit"], ev["won"], ev["lost"] = hit & at_agent, hit & at_opp, won, lost
            s[:, SA] += won
            s[:, SO] += lost
            reward = won.astype(np.int32) - lost.astype(np.int32)
            self._serve(won | lost)
            s[:, STEPS] += 1
            score = (s[:, SA] >= self.points) | (s[:, SO] >= self.points)
            trunc = ~score & (s[:, STEPS] >= self.max_steps)
        else:
            s[:, PA] = np.clip(s[:, PA] + move * CATCH_SPEED, 0, CATCH_PADDLE_MAX)
            x, vx = s[:, BX] + s[:, VX], s[:, VX].copy()
            low, high = x < 0, x > CATCH_BALL_MAX
            x = np.where(low, -x, np.where(high, 2 * CATCH_BALL_MAX - x, x))
            vx = np.where(low | high, -vx, vx)
            ev["wall"] = low | high
            y = np.minimum(s[:, BY] + CATCH_FALL, CATCH_PADDLE_Y - CATCH_BALL)
            s[:, BX], s[:, BY], s[:, VX] = x, y, vx
            landed = y >= CATCH_PADDLE_Y - CATCH_BALL
            caught = landed & (x + CATCH_BALL - 1 >= s[:, PA]) & (x <= s[:, PA] + CATCH_PADDLE_W - 1)
            ev["won"], ev["lost"] = caught, landed & ~caught
            s[:, SA] += ev["won"]
            s[:, SO] += ev["lost"]
            reward = ev["won"].astype(np.int32) - ev["lost"].astype(np.int32)
            s[:, STEPS] += 1
            score = landed
            trunc = ~score & (s[:, STEPS] >= self.max_steps)
        ev["score_done"], ev["trunc_done"] = score, trunc
        done = score | trunc
        self._new_episode(done)
        self.events = ev
        return self.render(), reward.astype(np.float32), done.astype(np.uint8)

    def rects(self):
        """The rectangles of each env as int32 [N][R][4] = (x0, x1, y0, y1), inclusive, from the clamped positions."""
        s = self.state
        n = self.N
        col = lambda v: np.full(n, v, np.int32)
        if self.game == PONG:
            pa, po = np.clip(s[:, PA], 0, PONG_PADDLE_MAX), np.clip(s[:, PO], 0, PONG_PADDLE_MAX)
            bx, by = np.clip(s[:, BX], 0, PONG_BALL_MAX), np.clip(s[:, BY], 0, PONG_BALL_MAX)
            r = [(col(PONG_OPP_X), col(PONG_OPP_X + 1), po, po + PONG_PADDLE_H - 1),
                 (col(PONG_AGENT_X), col(PONG_AGENT_X + 1), pa, pa + PONG_PADDLE_H - 1),
                 (bx, bx + PONG_BALL - 1, by, by + PONG_BALL - 1)]
        else:
            pa = np.clip(s[:, PA], 0, CATCH_PADDLE_MAX)
            bx, by = np.clip(s[:, BX], 0, CATCH_BALL_MAX), np.clip(s[:, BY], 0, CATCH_BALL_MAX)
            r = [(pa, pa + CATCH_PADDLE_W - 1, col(CATCH_PADDLE_Y), col(CATCH_PADDLE_Y + CATCH_PADDLE_H - 1)),
                 (bx, bx + CATCH_BALL - 1, by, by + CATCH_BALL - 1)]
        return np.stack([np.stack(q, axis=1) for q in r], axis=1).astype(np.int32)

    def render(self):
        """The frame is a pure function of the state: background 87, every pixel inside a rectangle 236."""
        rows = np.arange(SIZE, dtype=np.int32)[None, :, None]
        cols = np.arange(SIZE, dtype=np.int32)[None, None, :]
        inside = np.zeros((self.N, SIZE, SIZE), bool)
        r = self.rects()
        for q in range(r.shape[1]):
            x0, x1, y0, y1 = (r[:, q, j][:, None, None] for j in range(4))
            inside |= (cols >= x0) & (cols <= x1) & (rows >= y0) & (rows <= y1)
        return np.where(inside, OBJECT, BACKGROUND).astype(np.uint8)

    def is_reset_state(self):
        """[N] bool: the state is the first of an episode."""
        s = self.state
        if self.game == PONG:
            return ((s[:, BX] == PONG_SERVE_X) & (s[:, PA] == PONG_PADDLE_START) & (s[:, PO] == PONG_PADDLE_START) & (s[:, SA] == 0)
                    & (s[:, SO] == 0) & (s[:, STEPS] == 0))
        return (s[:, BY] == 0) & (s[:, PA] == CATCH_PADDLE_START) & (s[:, SA] == 0) & (s[:, SO] == 0) & (s[:, STEPS] == 0)


def tracking_actions(model):
    """The paddle-tracks-ball policy as float32 actions (1 = negative direction, 2 = positive direction, 0 = stay)."""
    s = model.state
    if model.game == PONG:
        off = s[:, BY] + 1 - (s[:, PA] + PONG_PADDLE_H // 2)
        return np.where(off < -1, 1, np.where(off > 1, 2, 0)).astype(np.float32)
    off = s[:, BX] + CATCH_BALL // 2 - (s[:, PA] + CATCH_PADDLE_W // 2)
    return np.where(off < -2, 1, np.where(off > 2, 2, 0)).astype(np.float32)


def coverage_run(game, seed):
    """The seeded coverage trajectory of the tests: (model kwargs, actions float32 [steps][N]).  Pong: N = 8, 400 steps, points = 2,
    max_steps = 150; Catch: N = 6, 64 steps; uniform actions in 0..5."""
    if game == "pong":
        n, steps, kw = 8, 400, dict(points=2, max_steps=150)
    else:
        n, steps, kw = 6, 64, dict()
    actions = np.random.default_rng(seed).integers(0, 6, size=(steps, n)).astype(np.float32)
    return dict(n_envs=n, seed=seed, **kw), actions


COVERAGE_SEEDS = {"pong": 7, "catch": 11}
COVERAGE_EVENTS = {"pong": EVENT_NAMES, "catch": ("wall", "won", "lost")}


def play(model, actions):
    """Steps `model` through actions [steps][N] from a reset; returns (counts of every event class, list of per-step
    (state copy, frame, reward, done))."""
    counts = {k: 0 for k in EVENT_NAMES}
    trace = []
    first = model.reset()
    for a in actions:
        frame, reward, done = model.step(a)
        for k in EVENT_NAMES:
            counts[k] += int(model.events[k].sum())
        trace.append((model.state.copy(), frame, reward, done))
    return counts, trace, first
