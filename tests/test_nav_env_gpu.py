"""The device navigation env on the GPU (csrc/navenv.hip, ddrl4nav_amd.env.DeviceNavEnv, runner/device_loop.collect_states) against the
integer model of tests/nav_env_ref.py: every state word, lidar range, vector entry, map cell, reward and done after every step, bit for
bit; then the closed loop -- a StateRollout driven by collect_states() with in-pool rendering against a StateRollout fed by the host
model through put_states -- down to every parameter after net.learn.  Run with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

import nav_env_ref as R
from arena_harness import (HOSTILE, LOSS_KEYS, SHAPES, assert_tape_equals, closed_loop, dev, filled, host, is_fill, make_net, play_env, record,
                           same, tape_from)

pytestmark = pytest.mark.gpu

# ---- 1. bit parity with the model -----------------------------------------------------------------------------------------------------------
# (N, n_obstacles, n_peds, env0); the first case is the coverage tape itself (test_nav_env_cpu.py), the others 40 steps with two
# steps of hostile actions and max_steps = 15, so every case holds truncations and new episodes
TAPE = (8, 10, 5, 0)
SWEEP = [(1, 10, 5, 0), (5, 0, 0, 3), (5, 10, 0, 1000), (67, 0, 5, 2 ** 32 - 67), (67, 3, 2, 12345), (1, 3, 2, 2 ** 32 - 1)]


@functools.lru_cache(maxsize=None)
def reference(case):
    """(model kwargs, the rule book's tape) of one case; never modified."""
    n, n_obs, n_peds, env0 = case
    if case == TAPE:
        kw = dict(R.COVERAGE)
        want = record(R.NavEnvRef(**kw), R.COVERAGE_STEPS, np.random.RandomState(0))
        assert all(want["events"][k].sum() >= 1 for k in R.EVENT_NAMES)
    else:
        kw = dict(n_envs=n, seed=100 + n, n_obstacles=n_obs, n_peds=n_peds, max_steps=15, env0=env0)
        want = record(R.NavEnvRef(**kw), 40, np.random.RandomState(n + n_obs), hostile={t: np.roll(HOSTILE, t, axis=0) for t in (7, 23)})
        assert want["events"]["trunc"].sum() >= 1 or n == 1
    return kw, want


def play_on_device(kw, actions, start=None):
    """The tape on a fresh DeviceNavEnv (arena_harness.play_env) and the env.  start: a state_dict to resume from instead of a reset."""
    from ddrl4nav_amd.env import DeviceNavEnv
    env = DeviceNavEnv(device="cuda", **kw)
    return play_env(env, actions, start), env


def check_against(case):
    kw, want = reference(case)
    assert_tape_equals(play_on_device(kw, want["actions"])[0], want)
    return want["reward"], want["done"]


def test_the_coverage_tape_equals_the_model():
    """N = 8, 300 steps: all 64 state words, 960 ranges, 5 vector floats, 6,912 map floats, reward and done after every step."""
    want_r, want_d = check_against(TAPE)
    assert want_d.sum() > 20 and (want_r > 14).any() and (want_r < -14).any()


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "N%d-obs%d-ped%d-env0_%d" % c)
def test_sweep_equals_the_model(case):
    want_r, want_d = check_against(case)
    assert want_d.any()


def test_repeats_are_bit_identical():
    kw, want = reference(SWEEP[4])
    assert_tape_equals(play_on_device(kw, want["actions"])[0], play_on_device(kw, want["actions"])[0])


def test_the_env_owns_its_outputs_by_default():
    from ddrl4nav_amd.env import DeviceNavEnv, make_device_env
    kw, want = reference(SWEEP[2])
    env = make_device_env({"env_name": "DeviceNav-v0", "env_num": kw["n_envs"], "env_seed": kw["seed"], "env_obstacles": 10,
                           "env_peds": 0, "env_max_steps": 15}, env0=kw["env0"])
    assert isinstance(env, DeviceNavEnv) and env.state_shapes == SHAPES
    out = env.reset()
    assert all(o is e for o, e in zip(out, env.obs)) and all(same(host(o), f) for o, f in zip(out, want["first"]))
    for t in range(10):
        o, r, d = env.step(dev(want["actions"][t]))
        assert all(x is e for x, e in zip(o, env.obs)) and r.dtype == torch.float32 and d.dtype == torch.uint8
    assert same(host(o[0]), want["laser"][9]) and same(host(o[2]), want["image"][9]) and np.array_equal(host(env.state), want["state"][9])


def test_masked_reset():
    """Only the envs with a non-zero mask byte restart (all counters zero, their first observation rendered); the others keep their
    state and their rows of the observation, whatever those hold."""
    from ddrl4nav_amd.env import DeviceNavEnv
    n = 5
    kw = dict(seed=9, env0=2, n_obstacles=4, n_peds=3, max_steps=50)
    model, env = R.NavEnvRef(n, **kw), DeviceNavEnv(n, device="cuda", **kw)
    model.reset()
    env.reset()
    rng = np.random.RandomState(4)
    for t in range(12):
        a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        model.step(a)
        env.step(dev(a))
    mask = np.array([0, 3, 0, 1, 255], np.uint8)
    before = model.state.copy()
    want = model.reset(mask)
    bufs = filled(3, n)
    got = env.reset(mask=dev(mask), obs_out=[b[1] for b in bufs])
    torch.cuda.synchronize()
    assert np.array_equal(host(env.state), model.state) and np.array_equal(model.state[[0, 2]], before[[0, 2]])
    assert (model.state[[1, 3, 4], R.STEPS] == 0).all() and (model.state[[1, 3, 4], R.EVENTS] == 3 + 4 + 3).all()
    for g, w, b in zip(got, want, bufs):
        assert same(host(g)[[1, 3, 4]], w[[1, 3, 4]]) and is_fill(g[0]) and is_fill(g[2]) and is_fill(b[0]) and is_fill(b[2])
    a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)                   # and the episodes go on for all five
    o, r, d = model.step(a)
    go, gr, gd = env.step(dev(a))
    assert np.array_equal(host(env.state), model.state) and all(same(host(x), y) for x, y in zip(go, o)) and same(host(gr), r)


def test_state_dict_resumes_bit_identically():
    from ddrl4nav_amd.env import DeviceNavEnv
    kw, want = reference(SWEEP[4])
    _, env = play_on_device(kw, want["actions"][:20])
    sd = env.state_dict()
    assert not sd["state"].is_cuda and sd["n_obstacles"] == 3 and sd["max_steps"] == 15
    got, _ = play_on_device(kw, want["actions"][20:], start=sd)         # a resumed env renders nothing before its first step: play_env
    assert_tape_equals(got, tape_from(want, 20))
    with pytest.raises(ValueError):
        DeviceNavEnv(device="cuda", **dict(kw, n_peds=3)).load_state_dict(sd)
    with pytest.raises(ValueError):
        DeviceNavEnv(device="cuda", **dict(kw, max_steps=16)).load_state_dict(sd)


@pytest.mark.parametrize("pops", [(10, 5), (3, 2), (0, 0)])
def test_a_hostile_state_is_sanitised(pops):
    """A state of random int32 words (and the extremes): the outputs equal the model's after sanitize(), nothing outside the env's rows
    is written, and the stored state is a sanitised one."""
    from ddrl4nav_amd.env import DeviceNavEnv
    n = 37
    kw = dict(seed=6, n_obstacles=pops[0], n_peds=pops[1], max_steps=40, env0=77)
    rng = np.random.RandomState(pops[0] + 1)
    words = rng.randint(-2 ** 31, 2 ** 31, size=(n, 64), dtype=np.int64).astype(np.int32)
    words[0], words[1], words[2] = np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1
    words[3:20, R.STEPS] = rng.randint(0, 30, 17)                       # some envs go on with their episode
    words[3:20, R.X:R.Y + 1] = rng.randint(-1500, 1500, (17, 2))
    model = R.NavEnvRef(n, **kw)
    want = record(model, 2, first_state=words, actions=rng.uniform(-1, 1, (2, n, 2)).astype(np.float32))
    assert_tape_equals(play_env(DeviceNavEnv(n, device="cuda", **kw), want["actions"], start=words), want)
    assert 0 < want["done"][0].sum() < n
    kept = model.state.copy()
    model.sanitize()
    assert np.array_equal(model.state, kept)


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from ddrl4nav_amd import ops
    from ddrl4nav_amd._lib import DdrlError
    from ddrl4nav_amd.env import DeviceNavEnv
    env = DeviceNavEnv(3, device="cuda")
    flat = torch.zeros(3 * 960 + 16, dtype=torch.float32, device="cuda")
    with pytest.raises(AssertionError):
        env.reset(obs_out=[flat[1:1 + 3 * 960].view(3, 1, 960), env.obs[1], env.obs[2]])     # a laser base that is not 16-byte aligned
    env.reset(obs_out=[flat[4:4 + 3 * 960].view(3, 1, 960), env.obs[1], env.obs[2]])
    with pytest.raises(AssertionError):
        env.step(torch.zeros((3, 2), dtype=torch.float64, device="cuda"))
    with pytest.raises(AssertionError):
        env.step(torch.zeros(3, dtype=torch.float32, device="cuda"))
    with pytest.raises(AssertionError):
        env.reset(obs_out=[env.obs[0], env.obs[1], torch.zeros((2, 3, 48, 48), device="cuda")])
    with pytest.raises(AssertionError):
        env.reset(mask=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(DdrlError):                                       # the reward inside the image
        ops.nav_env_step(env.state, torch.zeros((3, 2), device="cuda"), env.obs, env.obs[2].view(-1)[:3], env.done)
    with pytest.raises(DdrlError):
        ops.nav_env_step(env.state, torch.zeros((3, 2), device="cuda"), env.obs, env.reward, env.done, n_peds=6)


# ---- 2. the closed loop -----------------------------------------------------------------------------------------------------------------------
N, T = 4, 8
ENV_KW = dict(seed=31, n_obstacles=10, n_peds=5, max_steps=5)           # every env is done every fifth step: both rollouts see dones


@pytest.mark.parametrize("normalize_obs", [False, True])
def test_closed_loop_equals_the_host_driven_rollout(normalize_obs):
    """arena_harness.closed_loop on a DeviceNavEnv: collect_states() with in-pool rendering against the host model through put_states,
    two rollouts with carry_over() between them."""
    from ddrl4nav_amd.env import DeviceNavEnv
    out = closed_loop(DeviceNavEnv(N, device="cuda", **ENV_KW), R.NavEnvRef(N, **ENV_KW), T, normalize_obs=normalize_obs)
    assert out.dones[:T].any() and out.dones[T:].any() and out.dones.sum() >= 3 * N


@pytest.mark.parametrize("keep_step", [False, True])
def test_collect_states_honours_both_carry_over_modes(keep_step):
    """Three chained rollouts per mode: the env's trajectory is the model's under the actions the rollouts stored, in order, with no step
    played twice or skipped (keep_step: the bootstrap action is played and its reward recorded in row T; its observation waits in
    env.obs and becomes slot 1 of the next rollout)."""
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.env import DeviceNavEnv
    from ddrl4nav_amd.runner.device_loop import collect_states
    net = make_net(N * T, seed=5)
    ro = StateRollout(net, N, SHAPES, horizon=T)
    kw = dict(seed=13, n_obstacles=6, n_peds=4, max_steps=7)
    env, model = DeviceNavEnv(N, device="cuda", **kw), R.NavEnvRef(N, **kw)
    obs = model.reset()
    for r in range(3):
        collect_states(ro, env, keep_step=keep_step)
        torch.cuda.synchronize()
        assert ro.t0 == (1 if keep_step and r > 0 else 0)
        acts, rew, don = host(ro._actions), host(ro._rewards), host(ro._dones)
        for t in range(ro.t0, T + 1 if keep_step else T):
            assert all(same(host(p[t]), x) for p, x in zip(ro.states, obs)), (r, t)
            obs, reward, done = model.step(acts[t])
            assert same(rew[t], reward) and np.array_equal(don[t], done), (r, t)
        if not keep_step:
            assert all(same(host(p[T]), x) for p, x in zip(ro.states, obs))
        assert np.array_equal(host(env.state), model.state)
        ro.carry_over(keep_step=keep_step)
    with pytest.raises(ValueError):
        collect_states(ro, DeviceNavEnv(N + 1, device="cuda"))


def test_train_states_runs_three_updates():
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.env import DeviceNavEnv
    from ddrl4nav_amd.runner.device_loop import train_states
    net = make_net(N * T, seed=2)
    net.training_iter_time = 2
    ro = StateRollout(net, N, SHAPES, horizon=T, track_returns=True)
    env = DeviceNavEnv(N, device="cuda", seed=4, max_steps=6)
    start = net.params.clone()
    out = list(train_states(net, env, ro, 3))
    assert len(out) == 3 and ro.rollouts == 3 and not torch.equal(net.params, start)
    for losses, mean_return in out:
        assert all(np.isfinite(losses[k]) for k in LOSS_KEYS)
    assert -16.5 <= out[-1][1] <= 16.5      # 24 steps: every env has finished four episodes of at most 6 steps, 0.25 of progress each
