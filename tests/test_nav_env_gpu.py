"""The device navigation env on the GPU (csrc/navenv.hip, ddrl4nav_amd.env.DeviceNavEnv, runner/device_loop.collect_states) against the
integer model of tests/nav_env_ref.py: every state word, lidar range, vector entry, map cell, reward and done after every step, bit for
bit; then the closed loop -- a StateRollout driven by collect_states() with in-pool rendering against a StateRollout fed by the host
model through put_states -- down to every parameter after net.learn.  Run with `-m gpu`."""
import functools
import types

import numpy as np
import pytest
import torch

import nav_env_ref as R

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
SHAPES = [(1, 960), (5,), (3, 48, 48)]
HOSTILE = np.array([[np.nan, np.nan], [np.inf, np.inf], [-np.inf, -np.inf], [1e30, 1e30], [-5.0, -5.0], [np.inf, np.nan], [1e30, -1e30]],
                   np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    """float32 array -> its words: equality below is bitwise (a negative zero is not a zero)."""
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- 1. bit parity with the model -----------------------------------------------------------------------------------------------------------
# (N, n_obstacles, n_peds, env0); the first case is the coverage tape itself (test_nav_env_cpu.py), the others 40 steps with two
# steps of hostile actions and max_steps = 15, so every case holds truncations and new episodes
TAPE = (8, 10, 5, 0)
SWEEP = [(1, 10, 5, 0), (5, 0, 0, 3), (5, 10, 0, 1000), (67, 0, 5, 2 ** 32 - 67), (67, 3, 2, 12345), (1, 3, 2, 2 ** 32 - 1)]


@functools.lru_cache(maxsize=None)
def reference(case):
    """(model kwargs, actions [steps][n][2], first observation, per-step states / lasers / vectors / images / rewards / dones stacked) of
    one case; never modified."""
    n, n_obs, n_peds, env0 = case
    if case == TAPE:
        kw = dict(R.COVERAGE)
        counts, actions, first, trace = R.coverage_run()
        assert all(counts[k] >= 1 for k in R.EVENT_NAMES), counts
    else:
        kw = dict(n_envs=n, seed=100 + n, n_obstacles=n_obs, n_peds=n_peds, max_steps=15, env0=env0)
        hostile = {t: np.resize(np.roll(HOSTILE, t, axis=0), (n, 2)) for t in (7, 23)}
        counts, actions, first, trace = R.play(R.NavEnvRef(**kw), 40, np.random.RandomState(n + n_obs), hostile=hostile)
        assert counts["trunc"] >= 1 or n == 1
    stacked = (np.stack([s[0] for s in trace]),) + tuple(np.stack([s[1][k] for s in trace]) for k in range(3)) \
        + (np.stack([s[2] for s in trace]), np.stack([s[3] for s in trace]))
    return kw, actions, first, stacked


def guarded(rows, n):
    """Three fp32 buffers [rows, n, ...] filled with the guard word."""
    return [torch.full((rows, n) + s, GUARD, dtype=torch.int32, device="cuda").view(torch.float32) for s in SHAPES]


def is_guard(t):
    return bool((t.view(torch.int32) == GUARD).all())


def play_on_device(kw, actions, start=None):
    """The trajectory on a fresh DeviceNavEnv, every step rendered into its own row of three larger buffers (obs_out) with a guard row on
    either side; one read-back at the end.  start: a state_dict to resume from instead of a reset."""
    from ddrl4nav_amd.env import DeviceNavEnv
    steps, n = actions.shape[:2]
    env = DeviceNavEnv(device="cuda", **kw)
    env.state.fill_(-12345)                                             # reset reads nothing of what was there
    bufs = guarded(steps + 3, n)
    states = torch.empty((steps, n, 64), dtype=torch.int32, device="cuda")
    rewards = torch.empty((steps, n), dtype=torch.float32, device="cuda")
    dones = torch.empty((steps, n), dtype=torch.uint8, device="cuda")
    acts = dev(actions)
    if start is None:
        out = env.reset(obs_out=[b[1] for b in bufs])
        assert all(o.data_ptr() == b[1].data_ptr() for o, b in zip(out, bufs))
    else:
        env.load_state_dict(start)
    for t in range(steps):
        o, r, d = env.step(acts[t], obs_out=[b[t + 2] for b in bufs])
        assert all(x.data_ptr() == b[t + 2].data_ptr() for x, b in zip(o, bufs)) and r is env.reward and d is env.done
        states[t].copy_(env.state)
        rewards[t].copy_(r)
        dones[t].copy_(d)
    torch.cuda.synchronize()
    assert all(is_guard(b[0]) and is_guard(b[-1]) for b in bufs)         # nothing outside the rows that were handed over
    return [host(b) for b in bufs], host(states), host(rewards), host(dones), env


def check_against(case, steps=None):
    kw, actions, first, (want_s, want_l, want_v, want_i, want_r, want_d) = reference(case)
    steps = len(actions) if steps is None else steps
    (las, vec, img), states, rewards, dones, _ = play_on_device(kw, actions[:steps])
    assert same(las[1], first[0]) and same(vec[1], first[1]) and same(img[1], first[2])
    for t in range(steps):                                              # the first step that differs, if any, names itself
        assert np.array_equal(states[t], want_s[t]), (t, np.nonzero(states[t] != want_s[t]))
        assert same(rewards[t], want_r[t]) and np.array_equal(dones[t], want_d[t]), t
        assert same(las[t + 2], want_l[t]), (t, np.nonzero(las[t + 2] != want_l[t]))
        assert same(vec[t + 2], want_v[t]), t
        assert same(img[t + 2], want_i[t]), t
    return want_r, want_d


def test_the_coverage_tape_equals_the_model():
    """N = 8, 300 steps: all 64 state words, 960 ranges, 5 vector floats, 6,912 map floats, reward and done after every step."""
    want_r, want_d = check_against(TAPE)
    assert want_d.sum() > 20 and (want_r > 14).any() and (want_r < -14).any()


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "N%d-obs%d-ped%d-env0_%d" % c)
def test_sweep_equals_the_model(case):
    want_r, want_d = check_against(case)
    assert want_d.any()


def test_repeats_are_bit_identical():
    kw, actions, _, _ = reference(SWEEP[4])
    a, b = play_on_device(kw, actions)[:4], play_on_device(kw, actions)[:4]
    for x, y in zip(a[0], b[0]):
        assert same(x, y)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


def test_the_env_owns_its_outputs_by_default():
    from ddrl4nav_amd.env import DeviceNavEnv, make_device_env
    kw, actions, first, (want_s, want_l, want_v, want_i, want_r, want_d) = reference(SWEEP[2])
    env = make_device_env({"env_name": "DeviceNav-v0", "env_num": kw["n_envs"], "env_seed": kw["seed"], "env_obstacles": 10,
                           "env_peds": 0, "env_max_steps": 15}, env0=kw["env0"])
    assert isinstance(env, DeviceNavEnv) and env.state_shapes == SHAPES
    out = env.reset()
    assert all(o is e for o, e in zip(out, env.obs)) and all(same(host(o), f) for o, f in zip(out, first))
    for t in range(10):
        o, r, d = env.step(dev(actions[t]))
        assert all(x is e for x, e in zip(o, env.obs)) and r.dtype == torch.float32 and d.dtype == torch.uint8
    assert same(host(o[0]), want_l[9]) and same(host(o[2]), want_i[9]) and np.array_equal(host(env.state), want_s[9])


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
    bufs = guarded(3, n)
    got = env.reset(mask=dev(mask), obs_out=[b[1] for b in bufs])
    torch.cuda.synchronize()
    assert np.array_equal(host(env.state), model.state) and np.array_equal(model.state[[0, 2]], before[[0, 2]])
    assert (model.state[[1, 3, 4], R.STEPS] == 0).all() and (model.state[[1, 3, 4], R.EVENTS] == 3 + 4 + 3).all()
    for g, w, b in zip(got, want, bufs):
        assert same(host(g)[[1, 3, 4]], w[[1, 3, 4]]) and is_guard(g[0]) and is_guard(g[2]) and is_guard(b[0]) and is_guard(b[2])
    a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)                   # and the episodes go on for all five
    o, r, d = model.step(a)
    go, gr, gd = env.step(dev(a))
    assert np.array_equal(host(env.state), model.state) and all(same(host(x), y) for x, y in zip(go, o)) and same(host(gr), r)


def test_state_dict_resumes_bit_identically():
    from ddrl4nav_amd.env import DeviceNavEnv
    kw, actions, _, (want_s, want_l, want_v, want_i, want_r, want_d) = reference(SWEEP[4])
    *_, env = play_on_device(kw, actions[:20])
    sd = env.state_dict()
    assert not sd["state"].is_cuda and sd["n_obstacles"] == 3 and sd["max_steps"] == 15
    (las, vec, img), states, rewards, dones, _ = play_on_device(kw, actions[20:], start=sd)
    assert np.array_equal(states, want_s[20:]) and same(rewards, want_r[20:]) and np.array_equal(dones, want_d[20:])
    assert same(las[2:-1], want_l[20:]) and same(vec[2:-1], want_v[20:]) and same(img[2:-1], want_i[20:])
    assert is_guard(torch.from_numpy(las[1]))                           # a resumed env renders nothing before its first step
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
    model, env = R.NavEnvRef(n, **kw), DeviceNavEnv(n, device="cuda", **kw)
    model.state[:] = words
    env.state.copy_(dev(words))
    bufs = guarded(4, n)
    for t in range(2):
        a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        o, r, d = model.step(a)
        go, gr, gd = env.step(dev(a), obs_out=[b[t + 1] for b in bufs])
        assert np.array_equal(host(env.state), model.state), t
        assert all(same(host(x), y) for x, y in zip(go, o)) and same(host(gr), r) and np.array_equal(host(gd), d), t
        assert t > 0 or (0 < d.sum() < n)
    kept = model.state.copy()
    model.sanitize()
    assert np.array_equal(model.state, kept)
    assert all(is_guard(b[0]) and is_guard(b[3]) for b in bufs)


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
POOLS = ("_actions", "_logps", "values", "_dones", "_rewards", "adv", "ret")
LOSS_KEYS = ("PpoTotalLoss", "ActorLoss", "VLoss", "EntLoss")


def make_net(seed=13):
    """BASELINE config 4's net (NavPreNet1D x2 + GaussionActor(2)) through create_net, hashed weights loaded; two nets made by this
    function draw the same actions from the same observations."""
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.utils.recipe import hash_weights
    env = {"discrete_action": False, "act_dim": 2, "image_batch": 1, "ped_sim": {"total": 3}}
    cfg = BaseConfig(types.SimpleNamespace(task="test", ip="127.0.0.1"),
                     dict({"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8}, **env))
    cfg.TASK_TYPE = "robot_nav"
    cfg_nn = ConfigNN(env)
    cfg_nn.SHARE_CNN_NET = False
    torch.manual_seed(seed)
    net = create_net({"config": cfg, "config_nn": cfg_nn, "config_env": env}, max_batch=N * T)
    w = hash_weights([(k, tuple(p.shape)) for k, p in net.named_parameters()], seed)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    return net


def learn(net, ro):
    items = [({k: ld[k] for k in LOSS_KEYS}, ut) for ld, ut, _ in net.learn(ro.batch())]   # PpoBackUpTime is a wall clock
    assert items
    return items


def snapshot(ro):
    torch.cuda.synchronize()
    return {k: getattr(ro, k).clone() for k in POOLS}


@pytest.mark.parametrize("normalize_obs", [False, True])
def test_closed_loop_equals_the_host_driven_rollout(normalize_obs):
    """Variant A: StateRollout + DeviceNavEnv through collect_states(), the observation rendered in the pool.  Variant B: an identically
    seeded net whose StateRollout is fed by the host model through put_states, stepped with the actions read back.  Two rollouts with
    carry_over() between them."""
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.env import DeviceNavEnv
    from ddrl4nav_amd.nn import GenericPPO
    from ddrl4nav_amd.runner.device_loop import collect_states
    net_a, net_b = make_net(), make_net()
    assert isinstance(net_a, GenericPPO) and net_a.continuous
    ra = StateRollout(net_a, N, SHAPES, horizon=T, track_returns=True, normalize_obs=normalize_obs)
    rb = StateRollout(net_b, N, SHAPES, horizon=T, track_returns=True, normalize_obs=normalize_obs)
    assert [tuple(r.shape) for r in ra.state_rows(3)] == [(N,) + s for s in SHAPES]
    assert all(r.data_ptr() == p[3].data_ptr() for r, p in zip(ra.state_rows(3), ra.states))
    env = DeviceNavEnv(N, device="cuda", **ENV_KW)
    model = R.NavEnvRef(N, **ENV_KW)
    before = net_a.params.clone()
    all_r, all_d = [], []
    for r in range(2):
        collect_states(ra, env)
        if r == 0:
            rb.put_states(0, [dev(x) for x in model.reset()])
        for t in range(T):
            obs, reward, done = model.step(host(rb.act(t)))
            rb.record(t, reward, done)
            rb.put_states(t + 1, [dev(x) for x in obs])
            all_r.append(reward)
            all_d.append(done)
        rb.bootstrap()
        rb.finish()
        assert ra.rollouts == rb.rollouts == r + 1
        sa, sb = snapshot(ra), snapshot(rb)
        for k in POOLS:
            assert torch.equal(sa[k][:T], sb[k][:T]), (r, k)
        assert torch.equal(sa["values"], sb["values"])                   # the bootstrap row too
        assert np.array_equal(host(ra.dones), np.stack(all_d[-T:])) and same(host(ra.rewards), np.stack(all_r[-T:]))
        assert np.array_equal(host(env.state), model.state)
        for pa, pb in zip(ra.states, rb.states):                          # the pool rows hold the model's observations
            assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), r
        items_a, items_b = learn(net_a, ra), learn(net_b, rb)
        assert items_a == items_b
        assert torch.equal(net_a.params, net_b.params), r
        for (ka, pa), (kb, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
            assert ka == kb and torch.equal(pa, pb), (r, ka)
        ra.carry_over()
        rb.carry_over()
    assert not torch.equal(net_a.params, before)
    # ro.returns against the model's episode returns (Status.update_reward_status over the 2 T steps)
    rew, don = np.stack(all_r), np.stack(all_d)
    assert don[:T].any() and don[T:].any() and don.sum() >= 3 * N
    rsum, rep, fin = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32)
    for t in range(2 * T):
        rsum += rew[t]
        rep = np.where(don[t] != 0, rsum, rep)
        rsum = np.where(don[t] != 0, np.float32(0), rsum)
        fin += don[t] != 0
    for ro in (ra, rb):
        assert same(host(ro.returns.rewards_episode), rep) and np.array_equal(host(ro.returns.episodes_finished), fin)
        assert same(host(ro.returns.rewards_sum), rsum)
    assert ra.returns.mean_return() == float(rep[fin > 0].astype(np.float32).mean())


@pytest.mark.parametrize("keep_step", [False, True])
def test_collect_states_honours_both_carry_over_modes(keep_step):
    """Three chained rollouts per mode: the env's trajectory is the model's under the actions the rollouts stored, in order, with no step
    played twice or skipped (keep_step: the bootstrap action is played and its reward recorded in row T; its observation waits in
    env.obs and becomes slot 1 of the next rollout)."""
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.env import DeviceNavEnv
    from ddrl4nav_amd.runner.device_loop import collect_states
    net = make_net(seed=5)
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
    net = make_net(seed=2)
    net.training_iter_time = 2
    ro = StateRollout(net, N, SHAPES, horizon=T, track_returns=True)
    env = DeviceNavEnv(N, device="cuda", seed=4, max_steps=6)
    start = net.params.clone()
    out = list(train_states(net, env, ro, 3))
    assert len(out) == 3 and ro.rollouts == 3 and not torch.equal(net.params, start)
    for losses, mean_return in out:
        assert all(np.isfinite(losses[k]) for k in LOSS_KEYS)
    assert -16.5 <= out[-1][1] <= 16.5      # 24 steps: every env has finished four episodes of at most 6 steps, 0.25 of progress each
