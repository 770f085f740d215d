"""Host side of the device navigation env (tests/nav_env_ref.py, the rule book of csrc/navenv.hip): the library's trig table against the
formula, the model's self-checks and the event coverage of the tape the GPU test replays, the header against the binding table, and the
refusals of DeviceNavEnv, make_device_env, the ops wrappers and the C ABI.  No GPU."""
import functools
import itertools
import math
import os

import numpy as np
import pytest

import nav_env_ref as R
from arena_abi import BASE, ROOT, caller, common_refusals, header_declares, overlaps, refused, sizes

NEW = ("ddrl_op_nav_env_state_ints", "ddrl_op_nav_env_trig", "ddrl_op_nav_env_reset", "ddrl_op_nav_env_step")


@functools.lru_cache(maxsize=None)
def tape():
    return R.coverage_run()


# ---- 1. the trig table ----------------------------------------------------------------------------------------------------------------------
def test_the_library_table_is_the_formula_and_no_entry_is_near_a_tie():
    from ddrl4nav_amd import ops
    got = ops.nav_env_trig().numpy()
    assert got.shape == (2, 3840) and got.dtype == np.int32
    k = np.arange(3840, dtype=np.float64)
    for row, f, want in ((0, np.cos, R.COS), (1, np.sin, R.SIN)):
        exact = 16384.0 * f(2.0 * np.pi * k / 3840.0)
        assert np.array_equal(np.floor(exact + 0.5).astype(np.int64), want) and np.array_equal(got[row], want)
        tie = np.abs(exact - np.floor(exact) - 0.5)                     # distance of 16384 f(.) from a half-integer
        print(f.__name__, "nearest tie", tie.min())
        assert tie.min() > 1e-4
    assert got[0, 0] == 16384 and got[1, 960] == 16384 and got[0, 1920] == -16384 and got[1, 0] == 0
    gen = os.path.join(ROOT, "tools", "gen_nav_trig.py")
    ns = {"__file__": gen, "__name__": "gen_nav_trig"}
    exec(compile(open(gen).read(), gen, "exec"), ns)                    # the committed file is what the tool writes
    assert open(ns["OUT"]).read() == ns["text"]()


# ---- 2. the model -----------------------------------------------------------------------------------------------------------------------------
def test_isqrt_is_the_exact_floor():
    rng = np.random.default_rng(3)
    roots = rng.integers(0, 2 ** 28, 3000, dtype=np.int64)
    vals = np.concatenate([rng.integers(0, 2 ** 56, 1000, dtype=np.int64), roots * roots, roots * roots + 1, np.maximum(roots * roots - 1, 0),
                           np.array([0, 1, 2, 3, 4, 2 ** 56 - 1, 2 ** 56, (2 ** 28 - 1) ** 2, 2 ** 55 + 1], np.int64)])
    assert len(vals) >= 10 ** 4
    got = R.isqrt(vals)
    assert got.dtype == np.int64 and [int(g) for g in got] == [math.isqrt(int(v)) for v in vals]


def test_action_decoding():
    a = np.array([[0.0, 0.0], [1.0, 1.0], [0.999, -0.999], [0.5, 0.5], [np.nan, np.nan], [np.inf, np.inf], [-np.inf, -np.inf],
                  [1e30, 1e30], [-5.0, -5.0], [0.03, -0.01], [-0.0, -0.0]], np.float32)
    v, w = R.decode_actions(a)
    assert v.tolist() == [0, 32, 31, 16, 0, 0, 0, 32, 0, 0, 0]
    assert w.tolist() == [0, 64, -63, 32, 0, 0, 0, 64, -64, 0, 0]


def _check_layout(m, rows):
    """New-episode states `rows` of model m: obstacles apart from each other, from the robot's start and from the goal."""
    s = m.state[rows].astype(np.int64)
    o = s[:, R.OBS0:R.OBS0 + 3 * m.n_obstacles].reshape(len(s), m.n_obstacles, 3)
    for a, b in itertools.combinations(range(m.n_obstacles), 2):
        d2 = (o[:, a, 0] - o[:, b, 0]) ** 2 + (o[:, a, 1] - o[:, b, 1]) ** 2
        assert (d2 > (o[:, a, 2] + o[:, b, 2]) ** 2).all()
    for k in range(m.n_obstacles):
        for px, py in ((s[:, R.X], s[:, R.Y]), (s[:, R.GX], s[:, R.GY])):
            assert ((o[:, k, 0] - px) ** 2 + (o[:, k, 1] - py) ** 2 > (o[:, k, 2] + R.ROBOT_R) ** 2).all()
    assert ((o[:, :, 2] >= R.OBS_R_MIN) & (o[:, :, 2] <= R.OBS_R_MAX)).all()
    p = s[:, R.PED0:R.PED0 + 4 * m.n_peds].reshape(len(s), m.n_peds, 4)
    assert ((p[:, :, 3] >= R.SPEED_MIN) & (p[:, :, 3] <= R.SPEED_MAX) & (p[:, :, 2] >= 0) & (p[:, :, 2] < R.HEADINGS)).all()
    assert (s[:, R.STEPS] == 0).all() and (s[:, R.V] == 0).all() and (s[:, R.W] == 0).all()
    assert (s[:, R.DPREV] == R.isqrt((s[:, R.GX] - s[:, R.X]) ** 2 + (s[:, R.GY] - s[:, R.Y]) ** 2)).all()


def test_model_invariants_over_seeded_play():
    """sanitize() is a no-op on every state the rules produce, every new episode is laid out without overlaps, the observation is a pure
    function of the state with exact values, and the discriminants stay far inside int64."""
    n, steps = 8, 160
    m = R.NavEnvRef(n, seed=5, max_steps=60)
    rng = np.random.RandomState(11)
    obs = m.reset()
    _check_layout(m, np.arange(n))
    dones = 0
    for t in range(steps):
        a = np.stack([rng.uniform(0.3, 1.0, n), rng.uniform(-1.0, 1.0, n)], axis=1).astype(np.float32)
        a[0::2] = R.steering_actions(obs[1])[0::2]
        events_before = m.state[:, R.EVENTS].copy()
        obs, reward, done = m.step(a)
        before = m.state.copy()
        m.sanitize()
        assert np.array_equal(m.state, before)
        laser, vector, image = obs
        assert laser.shape == (n, 1, 960) and vector.shape == (n, 5) and image.shape == (n, 3, 48, 48)
        assert all(x.dtype == np.float32 for x in obs) and reward.dtype == np.float32 and done.dtype == np.uint8
        assert (laser >= 0).all() and (laser <= 6.0).all() and np.array_equal(laser * 256, np.round(laser * 256))
        assert np.isin(image[:, 0], (0.0, 1.0)).all() and (np.abs(image[:, 1:]) <= 0.75).all()
        assert np.array_equal(reward * 256, np.round(reward * 256)) and (np.abs(reward) <= 15.5).all()
        for x, y in zip(obs, m.observe()):
            assert np.array_equal(x, y)
        fin = done != 0
        if fin.any():
            _check_layout(m, np.nonzero(fin)[0])
            assert (m.state[fin, R.EVENTS] >= events_before[fin] + 3 + m.n_obstacles + m.n_peds).all()
        assert ((m.state[:, R.STEPS] >= 0) & (m.state[:, R.STEPS] < m.max_steps)).all() and (m.state[:, R.USED:] == 0).all()
        dones += int(fin.sum())
    assert dones > 0
    print("largest discriminant: 2^%.1f" % math.log2(m.max_disc))
    assert 0 < m.max_disc < 2 ** 62
    # the bound over any sanitised state: |m| <= 2 * 2560 * sqrt(2), |d| < 16385 * sqrt(2) per component pair
    worst = (2 * R.ARENA_R * 2 * 16384) ** 2 + ((2 * (2 * R.ARENA_R) ** 2) << 28)
    assert worst < 2 ** 62


def test_unused_slots_stay_zero_and_populations_shape_the_draws():
    for n_obs, n_peds in ((0, 0), (10, 0), (0, 5), (3, 2)):
        m = R.NavEnvRef(4, seed=2, n_obstacles=n_obs, n_peds=n_peds, max_steps=9)
        m.reset()
        assert (m.state[:, R.EVENTS] == 3 + n_obs + n_peds).all()
        rng = np.random.RandomState(1)
        for t in range(20):
            obs, _, _ = m.step(rng.uniform(-1, 1, (4, 2)).astype(np.float32))
            assert (m.state[:, R.OBS0 + 3 * n_obs:R.PED0] == 0).all() and (m.state[:, R.PED0 + 4 * n_peds:] == 0).all()
            if n_peds == 0:
                assert not obs[2].any()


def test_a_shard_plays_the_games_of_the_single_process():
    n, a, b = 7, 2, 5
    kw = dict(seed=21, max_steps=30)
    whole, part = R.NavEnvRef(n, **kw), R.NavEnvRef(b - a, env0=a, **kw)
    for x, y in zip(whole.reset(), part.reset()):
        assert np.array_equal(x[a:b], y)
    rng = np.random.RandomState(2)
    for t in range(60):
        act = np.stack([rng.uniform(0.3, 1.0, n), rng.uniform(-1.0, 1.0, n)], axis=1).astype(np.float32)
        ow, rw, dw = whole.step(act)
        op, rp, dp = part.step(act[a:b])
        assert np.array_equal(whole.state[a:b], part.state) and all(np.array_equal(x[a:b], y) for x, y in zip(ow, op))
        assert np.array_equal(rw[a:b], rp) and np.array_equal(dw[a:b], dp)


def test_the_coverage_tape_holds_every_event_class():
    """The tape the GPU test replays: N = 8, 300 steps, seed 7, 10 obstacles, 5 pedestrians, max_steps = 120; even envs steer to the goal,
    odd envs act at random.  The counts are this model's own."""
    assert R.COVERAGE == dict(n_envs=8, seed=7, n_obstacles=10, n_peds=5, max_steps=120) and R.COVERAGE_STEPS == 300
    counts, actions, first, trace = tape()
    print(counts)
    assert actions.shape == (300, 8, 2) and len(trace) == 300
    assert (actions[:, 1::2, 0] >= 0.3).all() and np.isin(actions[:, 0::2, 0], np.float32([1.0, 0.2])).all()
    for k in R.EVENT_NAMES:
        assert counts[k] >= 1, (k, counts)
    assert counts == {"ped_turn": 124, "obstacle_hit": 10, "ped_hit": 7, "wall_hit": 3, "goal": 10, "trunc": 4}
    rewards = np.stack([step[2] for step in trace])
    assert (rewards > 14).any() and (rewards < -14).any()


def test_steering_beats_random_play():
    """The learnable gap: the goal-seeking policy collects more reward per env than uniform actions do."""
    total = {}
    rng = np.random.RandomState(5)
    for policy in ("steer", "random"):
        m = R.NavEnvRef(8, seed=3, max_steps=200)
        obs, tot = m.reset(), 0.0
        for t in range(200):
            a = R.steering_actions(obs[1]) if policy == "steer" else np.stack([rng.uniform(0.3, 1.0, 8), rng.uniform(-1.0, 1.0, 8)], axis=1)
            obs, r, _ = m.step(a.astype(np.float32))
            tot += float(r.sum())
        total[policy] = tot / 8
    print(total)
    assert total["steer"] > total["random"] + 10


# ---- 3. header, binding, wrappers -------------------------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_binds():
    from ddrl4nav_amd import ops
    _, lib = header_declares(NEW, [0, 1, 11, 14])
    assert lib.ddrl_op_nav_env_state_ints() == R.STATE_INTS == ops.nav_env_state_ints() == 64
    assert lib.ddrl_op_nav_env_trig(None) == -1
    assert ops.ENV_GAMES == {"pong": 0, "catch": 1}                    # the nav env is no third game
    assert all(hasattr(ops, k) for k in ("nav_env_state_ints", "nav_env_trig", "nav_env_reset", "nav_env_step"))


def test_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses: every refusal below is decided before the first HIP call."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    size, obs = sizes("ddrl_op_nav_env_reset"), ("st", "la", "ve", "im")
    bad = [{p: None} for p in obs] + [dict(n=0), dict(n=-4), dict(e0=-1), dict(e0=2 ** 32 - 7), dict(e0=2 ** 32), dict(nobs=-1),
                                      dict(nobs=11), dict(nped=-1), dict(nped=6)]
    bad += [dict(st=BASE["st"] + 4), dict(la=BASE["la"] + 8), dict(la=BASE["la"] + 4), dict(im=BASE["im"] + 1), dict(im=BASE["im"] + 8),
            dict(ve=BASE["ve"] + 2)]
    bad += overlaps(obs, size)
    bad += [{"mask": BASE[p]} for p in obs] + [{"mask": BASE[p] + size[p] - 1} for p in obs]
    bad += [{"mask": BASE["st"] - 7}]                                   # ending inside the state
    refused(caller(lib, "ddrl_op_nav_env_reset"), bad)
    refused(caller(lib, "ddrl_op_nav_env_step"), common_refusals("ddrl_op_nav_env_step") + [dict(n=0), dict(n=-1), dict(e0=2 ** 32 - 7)])



def test_device_nav_env_refuses_bad_arguments():
    from ddrl4nav_amd.env import DeviceNavEnv, make_device_env
    assert DeviceNavEnv.state_shapes == [(1, 960), (5,), (3, 48, 48)]
    for args, kw in (((0,), {}), ((-2,), {}), ((4,), dict(n_obstacles=11)), ((4,), dict(n_obstacles=-1)), ((4,), dict(n_peds=6)),
                     ((4,), dict(n_peds=-1)), ((4,), dict(max_steps=0)), ((4,), dict(seed=-1)), ((4,), dict(seed=2 ** 32)),
                     ((4,), dict(env0=-1)), ((4,), dict(env0=2 ** 32 - 3))):
        with pytest.raises(ValueError):
            DeviceNavEnv(*args, **kw)
    for cfg in ({"env_name": "DeviceNav-v1", "env_num": 4}, {"env_name": "DeviceNav-v0"}, {"env_name": "DeviceNav-v0", "env_num": 0},
                {"env_name": "DeviceNav-v0", "env_num": 4, "env_obstacles": 11}, {"env_name": "DeviceNav-v0", "env_num": 4, "env_peds": 6},
                {"env_name": "DeviceNav-v0", "env_num": 4, "env_max_steps": 0}, {"env_name": "DeviceNav-v0", "env_num": 4, "env_seed": -1},
                {"env_name": "PongNoFrameskip-v4", "env_num": 4}, {"env_num": 4}):
        with pytest.raises(ValueError):
            make_device_env(cfg)


def test_ops_wrappers_refuse_host_tensors():
    import torch
    from ddrl4nav_amd import ops
    st = torch.zeros((4, 64), dtype=torch.int32)
    obs = [torch.zeros((4,) + s) for s in ops.NAV_ENV_SHAPES]
    with pytest.raises(AssertionError):
        ops.nav_env_reset(st, obs)
    with pytest.raises(AssertionError):
        ops.nav_env_step(st, torch.zeros((4, 2)), obs, torch.zeros(4), torch.zeros(4, dtype=torch.uint8))


def test_state_rollout_and_loop_additions_exist():
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.runner import device_loop
    assert callable(StateRollout.state_rows) and callable(StateRollout.put_states_in_place)
    assert callable(device_loop.collect_states) and callable(device_loop.train_states)
