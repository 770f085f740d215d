"""Host side of the device environments (tests/device_env_ref.py, the rule book of csrc/denv.hip): the model's invariants and event
coverage over seeded random play, sharding by env0, the header against the binding table, and the refusals of DeviceEnv,
make_device_env, the ops wrappers and the C ABI.  No GPU."""
import os
import re

import numpy as np
import pytest

import device_env_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddrl_op_env_state_ints", "ddrl_op_env_reset", "ddrl_op_env_step")


# ---- 1. the model ---------------------------------------------------------------------------------------------------------------------------
def _check_ranges(m):
    s = m.state
    if m.game == R.PONG:
        assert ((s[:, R.BX] >= 0) & (s[:, R.BX] <= 82) & (s[:, R.BY] >= 0) & (s[:, R.BY] <= 82)).all()
        assert (np.abs(s[:, R.VX]) == 2).all() and (np.abs(s[:, R.VY]) <= 3).all()
        assert ((s[:, R.PA] >= 0) & (s[:, R.PA] <= 74) & (s[:, R.PO] >= 0) & (s[:, R.PO] <= 74)).all()
        assert ((s[:, R.SA] >= 0) & (s[:, R.SA] < m.points) & (s[:, R.SO] >= 0) & (s[:, R.SO] < m.points)).all()
    else:
        assert ((s[:, R.BX] >= 0) & (s[:, R.BX] <= 80) & (s[:, R.BY] >= 0) & (s[:, R.BY] <= 72) & (s[:, R.BY] % 4 == 0)).all()
        assert (np.abs(s[:, R.VX]) <= 1).all() and (s[:, R.VY] == 4).all() and ((s[:, R.PA] >= 0) & (s[:, R.PA] <= 72)).all()
    assert ((s[:, R.STEPS] >= 0) & (s[:, R.STEPS] < m.max_steps)).all() and (s[:, 10:] == 0).all()


@pytest.mark.parametrize("game,n,steps,kw", [("pong", 16, 1000, dict(points=3, max_steps=300)), ("catch", 16, 500, dict()),
                                             ("catch", 4, 100, dict(max_steps=7))])
def test_invariants_over_long_random_play(game, n, steps, kw):
    m = R.DeviceEnvRef(game, n, seed=5, **kw)
    rng = np.random.default_rng(17)
    frame = m.reset()
    assert m.is_reset_state().all()
    objects = {R.PONG: 2 * 20 + 4, R.CATCH: 24 + 16}[m.game]
    dones = 0
    for t in range(steps):
        events_before = m.state[:, R.EVENTS].copy()
        frame, reward, done = m.step(rng.integers(0, 6, n).astype(np.float32))
        _check_ranges(m)
        assert reward.dtype == np.float32 and done.dtype == np.uint8 and frame.dtype == np.uint8 and frame.shape == (n, 84, 84)
        assert np.isin(reward, (-1.0, 0.0, 1.0)).all() and np.isin(done, (0, 1)).all()
        assert m.is_reset_state()[done != 0].all()                      # done implies the first state of a new episode
        assert np.isin(frame, (R.BACKGROUND, R.OBJECT)).all()
        assert ((frame == R.OBJECT).sum(axis=(1, 2)) <= objects).all() and ((frame == R.OBJECT).sum(axis=(1, 2)) >= objects - 16).all()
        assert np.array_equal(frame, m.render())                        # a pure function of the state
        assert (m.state[:, R.EVENTS] >= events_before).all() and (m.state[:, R.EVENTS][done != 0] > events_before[done != 0]).all()
        dones += int(done.sum())
    assert dones > 0


@pytest.mark.parametrize("game", ["pong", "catch"])
def test_seeded_trajectory_covers_every_event_class(game):
    """The trajectory the GPU parity tests replay: every class of event the rules know occurs in it."""
    kw, actions = R.coverage_run(game, R.COVERAGE_SEEDS[game])
    assert (kw["n_envs"], len(actions)) == {"pong": (8, 400), "catch": (6, 64)}[game]
    if game == "pong":
        assert kw["points"] == 2 and kw["max_steps"] == 150
    assert actions.min() == 0 and actions.max() == 5
    counts, trace, first = R.play(R.DeviceEnvRef(game, **kw), actions)
    print(game, counts)
    for k in R.COVERAGE_EVENTS[game]:
        assert counts[k] >= 1, (k, counts)
    assert first.shape == (kw["n_envs"], 84, 84) and len(trace) == len(actions)


def test_first_frames():
    m = R.DeviceEnvRef("pong", 3, seed=1)
    f = m.reset()
    for i in range(3):
        by = m.state[i, R.BY]
        want = np.full((84, 84), 87, np.uint8)
        want[37:47, 4:6] = 236
        want[37:47, 78:80] = 236
        want[by:by + 2, 41:43] = 236
        assert np.array_equal(f[i], want)
    c = R.DeviceEnvRef("catch", 3, seed=1)
    f = c.reset()
    for i in range(3):
        bx = c.state[i, R.BX]
        want = np.full((84, 84), 87, np.uint8)
        want[80:82, 36:48] = 236
        want[0:4, bx:bx + 4] = 236
        assert np.array_equal(f[i], want)
    assert len({tuple(r) for r in m.state[:, :4]}) > 1                  # the envs' serves differ


def test_hash_is_a_fixed_function():
    """Pinned words of the hash (computed by hand from its definition in Python integers)."""
    def py(seed, env, c):
        x = (seed ^ (env * 0x9E3779B1) ^ (c * 0x85EBCA77)) & 0xFFFFFFFF
        for mul in (0x7FEB352D, 0x846CA68B):
            x ^= x >> 16
            x = (x * mul) & 0xFFFFFFFF
        return x ^ (x >> 16)
    for seed, env, c in ((0, 0, 0), (7, 3, 11), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (123456789, 4000000000, 77)):
        assert int(R.hash32(seed, np.array([env], np.uint32), np.array([c], np.uint32))[0]) == py(seed, env, c)
    assert py(0, 0, 0) == 0 and py(7, 3, 11) != py(7, 3, 12) != py(7, 4, 11)


def test_action_decoding():
    a = np.array([0, 1, 2, 3, 4, 5, 2.5, 5.9, np.nan, np.inf, -np.inf, -1, -0.5, 6.0, 1e30, 17, 18], np.float32)
    assert R.decode_actions(a, 6).tolist() == [0, 1, 2, 0, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert R.decode_actions(a, 18).tolist() == [0, 1, 2, 0, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 2, 0]
    assert R.decode_actions(a, 2).tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("game", ["pong", "catch"])
def test_a_shard_plays_the_games_of_the_single_process(game):
    """Envs [a, b) of a model with env0 = 0 equal a model of b - a envs with env0 = a."""
    n, a, b = 12, 5, 9
    kw = dict(seed=21, points=2, max_steps=90)
    whole, part = R.DeviceEnvRef(game, n, **kw), R.DeviceEnvRef(game, b - a, env0=a, **kw)
    assert np.array_equal(whole.reset()[a:b], part.reset())
    rng = np.random.default_rng(2)
    for t in range(200):
        act = rng.integers(0, 6, n).astype(np.float32)
        fw, rw, dw = whole.step(act)
        fp, rp, dp = part.step(act[a:b])
        assert np.array_equal(whole.state[a:b], part.state) and np.array_equal(fw[a:b], fp)
        assert np.array_equal(rw[a:b], rp) and np.array_equal(dw[a:b], dp)


def test_tracking_beats_random_play():
    """The learnable gap: per 1,000 steps random play loses points at Pong and the tracking paddle loses none; at Catch random play
    misses most balls and tracking catches every one."""
    out = {}
    for game in ("pong", "catch"):
        for policy in ("random", "track"):
            m = R.DeviceEnvRef(game, 16, seed=3)
            m.reset()
            rng = np.random.default_rng(5)
            total, lost = 0.0, 0
            for t in range(1000):
                a = rng.integers(0, 6, 16).astype(np.float32) if policy == "random" else R.tracking_actions(m)
                _, r, _ = m.step(a)
                total += float(r.sum())
                lost += int(m.events["lost"].sum())
            out[game, policy] = (total / 16, lost)
    print(out)
    assert out["pong", "track"][1] == 0 and out["catch", "track"][1] == 0
    assert out["pong", "random"][0] < -5 and out["catch", "random"][0] < -10 and out["catch", "track"][0] > 45


# ---- 2. header, binding, wrappers -------------------------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_binds():
    from ddrl4nav_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    for name in NEW:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        args = 0 if m.group(1).strip() == "void" else m.group(1).count(",") + 1
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == args, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [0, 8, 13]
    assert re.search(r"#define\s+DDRL_ABI_VERSION\s+3\b", text) and _lib.ABI_VERSION == 3
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW)
    assert lib.ddrl_op_env_state_ints() == R.STATE_INTS == ops.env_state_ints() == 16
    assert ops.ENV_GAMES == R.GAMES and hasattr(ops, "env_reset") and hasattr(ops, "env_step")


def test_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses: every refusal below is decided before the first HIP call."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    INVALID = -1
    a, M = 0x10000000, 0x1000000

    def reset(game=0, st=a, n=8, env0=0, seed=1, mask=None, fr=a + M):
        return lib.ddrl_op_env_reset(game, st, n, env0, seed, mask, fr, None)

    for kw in (dict(game=2), dict(game=-1), dict(st=None), dict(fr=None), dict(n=0), dict(n=-4), dict(env0=-1), dict(env0=2 ** 32 - 7),
               dict(st=a + 4), dict(fr=a + M + 8), dict(fr=a + M + 1),
               dict(fr=a + 16), dict(st=a + M + 7056 * 8 - 16),               # the frame inside the state, the state inside the frame
               dict(mask=a + 32), dict(mask=a + M + 7056 * 8 - 1), dict(mask=a - 7)):   # the mask inside the state, the frame, ending in the state
        assert reset(**kw) == INVALID, kw

    def step(game=0, st=a, n=8, env0=0, na=6, pts=21, ms=10000, seed=1, act=a + M, fr=a + 2 * M, rw=a + 3 * M, dn=a + 4 * M):
        return lib.ddrl_op_env_step(game, st, n, env0, na, pts, ms, seed, act, fr, rw, dn, None)

    for kw in (dict(game=2), dict(st=None), dict(act=None), dict(fr=None), dict(rw=None), dict(dn=None), dict(n=0), dict(n=-1),
               dict(env0=-3), dict(env0=2 ** 32), dict(na=1), dict(na=19), dict(na=0), dict(pts=0), dict(ms=0), dict(ms=-5),
               dict(st=a + 8), dict(fr=a + 2 * M + 4), dict(act=a + M + 2), dict(rw=a + 3 * M + 1),
               dict(fr=a), dict(fr=a + 496), dict(rw=a + 64), dict(dn=a + 511), dict(dn=a + 2 * M + 7056 * 8 - 1),
               dict(rw=a + 2 * M + 16), dict(dn=a + 3 * M + 31), dict(act=a + 64), dict(act=a + 2 * M + 32), dict(act=a + 3 * M + 28),
               dict(act=a + 4 * M + 4)):
        assert step(**kw) == INVALID, kw


def test_device_env_refuses_bad_arguments():
    from ddrl4nav_amd.env import DeviceEnv, make_device_env
    for args, kw in ((("tennis", 4), {}), (("pong", 0), {}), (("pong", -2), {}), (("pong", 4), dict(n_actions=1)),
                     (("pong", 4), dict(n_actions=19)), (("catch", 4), dict(points=0)), (("catch", 4), dict(max_steps=0)),
                     (("pong", 4), dict(seed=-1)), (("pong", 4), dict(seed=2 ** 32)), (("pong", 4), dict(env0=-1)),
                     (("pong", 4), dict(env0=2 ** 32 - 3))):
        with pytest.raises(ValueError):
            DeviceEnv(*args, **kw)
    for cfg in ({"env_name": "PongNoFrameskip-v4", "env_num": 4}, {"env_num": 4}, {"env_name": "DevicePong-v0"},
                {"env_name": "DeviceCatch-v0", "env_num": 0}, {"env_name": "DevicePong-v0", "env_num": 4, "discrete_actions": [0]},
                {"env_name": "DevicePong-v0", "env_num": 4, "env_points": 0}, {"env_name": "DevicePong-v0", "env_num": 4, "env_max_steps": 0}):
        with pytest.raises(ValueError):
            make_device_env(cfg)


def test_ops_wrappers_refuse_host_tensors_and_unknown_games():
    import torch
    from ddrl4nav_amd import ops
    st = torch.zeros((4, 16), dtype=torch.int32)
    fr = torch.zeros((4, 84, 84), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.env_reset("tennis", st, fr)
    with pytest.raises(AssertionError):
        ops.env_reset("pong", st, fr)                                  # host tensors
    with pytest.raises(AssertionError):
        ops.env_step("catch", st, torch.zeros(4), fr, torch.zeros(4), torch.zeros(4, dtype=torch.uint8))
