"""The multi-robot navigation env on the GPU (csrc/fleetenv.hip, ddrl4nav_amd.env.FleetNavEnv, runner/device_loop.collect_states)
against the integer model of tests/fleet_env_ref.py: every state word, lidar range, vector entry, map cell, reward, done and info word
after every step, bit for bit; hostile and hand-built states; NavStatus fed the device's info words; then the closed loop -- a
StateRollout driven by collect_states() with in-pool rendering against a StateRollout fed by the host model through put_states -- down to
every parameter after net.learn.  Run with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

import fleet_env_ref as F
import nav_env_ref as R
import nav_status_ref as S
from arena_harness import (HOSTILE, LOSS_KEYS, SHAPES, assert_status_equals, assert_tape_equals, close_to, closed_loop, dev, filled, host,
                           is_fill, make_net, play_env, record, same, tape_from)

pytestmark = pytest.mark.gpu

# ---- 1. bit parity with the model -----------------------------------------------------------------------------------------------------------
# (n_worlds, R, n_obstacles, n_peds, world0); the first case is the coverage tape itself (test_fleet_env_cpu.py), the others 40 steps with
# two steps of hostile actions and max_steps = 15, so every case holds truncations and respawns
TAPE = (6, 4, 10, 5, 0)
SWEEP = [(1, 1, 10, 5, 2 ** 32 - 1), (1, 4, 0, 0, 3), (5, 2, 10, 0, 1000), (17, 3, 0, 5, 12345), (67, 4, 3, 2, 2 ** 32 - 67)]


@functools.lru_cache(maxsize=None)
def reference(case):
    """(model kwargs, the rule book's tape) of one case; never modified."""
    nw, nr, n_obs, n_peds, world0 = case
    if case == TAPE:
        kw = dict(F.COVERAGE)
        want = record(F.FleetEnvRef(**kw), F.COVERAGE_STEPS, np.random.RandomState(0))
        assert all(want["events"][k].sum() >= 3 for k in F.EVENT_NAMES)
    else:
        kw = dict(n_worlds=nw, n_robots=nr, seed=100 + nw, n_obstacles=n_obs, n_peds=n_peds, max_steps=15, world0=world0)
        want = record(F.FleetEnvRef(**kw), 40, np.random.RandomState(nw + n_obs), hostile={t: np.roll(HOSTILE, t, axis=0) for t in (7, 23)})
        assert want["events"]["trunc"].sum() >= 1
    return kw, want


def play_on_device(kw, actions, start=None, emit_info=True):
    """The tape on a fresh FleetNavEnv (arena_harness.play_env) and the env.  start: a state_dict to resume from instead of a reset."""
    from ddrl4nav_amd.env import FleetNavEnv
    env = FleetNavEnv(device="cuda", emit_info=emit_info, **kw)
    assert env.N == env.n_worlds * env.n_robots and tuple(env.state.shape) == (env.n_worlds, 96)
    return play_env(env, actions, start), env


def check_against(case):
    kw, want = reference(case)
    assert_tape_equals(play_on_device(kw, want["actions"])[0], want)
    return want["reward"], want["done"], want["info"]


def test_the_coverage_tape_equals_the_model():
    """6 worlds x 4 robots, 300 steps: all 96 state words, 960 ranges, 5 vector floats, 6,912 map floats, reward, done and info word of
    every row after every step."""
    want_r, want_d, want_w = check_against(TAPE)
    assert want_d.sum() > 60 and (want_r > 14).any() and (want_r < -14).any()
    assert (S.unpack_info(want_w)["collision"] == 3).sum() >= 3


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "W%d-R%d-obs%d-ped%d-world0_%d" % c)
def test_sweep_equals_the_model(case):
    want_r, want_d, _ = check_against(case)
    assert want_d.any()


def test_one_robot_per_world_is_the_nav_kernel():
    """The device twin of test_fleet_env_cpu.py::test_one_robot_per_world_is_the_nav_rule_book: 4 worlds of one robot against 4 envs, same
    seed, same actions from [0, 1] x [-1, 1] -- the two kernels' shared pieces (csrc/navcore.h) against each other, not each against its
    own model.  After the reset and after each of 6 steps the laser, vector, image, reward, done, info word and every mapped state word
    are equal bit for bit.  No episode can end in 6 steps (so the two envs' different new-episode rules stay out of it): every obstacle
    centre and goal starts >= 608 - 128 sqrt(2) = 427 ticks from the robot, which moves <= 32 a step against a collision distance
    <= 192 and a goal tolerance of 77; a pedestrian starts >= 608 away and closes <= 56 a step against 141; the wall is >= 2,496 - 1,720
    away; max_steps is 500.  Populations (10, 5), (0, 0) and (3, 2)."""
    for n_obs, n_peds in ((10, 5), (0, 0), (3, 2)):
        _one_robot_against_nav(n_obs, n_peds)


def _one_robot_against_nav(n_obs, n_peds):
    from ddrl4nav_amd import ops
    n, steps = 4, 6
    kw = dict(seed=11, n_obstacles=n_obs, n_peds=n_peds)
    make = lambda: ([torch.empty((n,) + s, dtype=torch.float32, device="cuda") for s in SHAPES],
                    torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"),
                    torch.empty(n, dtype=torch.int32, device="cuda"))
    (fo, fr, fd, fw), (no, nr, nd, nw) = make(), make()
    fs = torch.full((n, 96), -12345, dtype=torch.int32, device="cuda")
    ns = torch.full((n, 64), -12345, dtype=torch.int32, device="cuda")
    ops.fleet_env_reset(fs, 1, fo, world0=5, **kw)
    ops.nav_env_reset(ns, no, env0=5, **kw)

    def compare(t):
        assert np.array_equal(F.nav_state(host(fs)), host(ns)), (t, np.nonzero(F.nav_state(host(fs)) != host(ns)))
        for name, a, b in zip(("laser", "vector", "image"), fo, no):
            assert same(host(a), host(b)), (t, name)

    compare("reset")
    actions = np.random.RandomState(n_obs + 7).uniform([0.0, -1.0], [1.0, 1.0], (steps, n, 2)).astype(np.float32)
    for t in range(steps):
        a = dev(actions[t])
        ops.fleet_env_step(fs, 1, a, fo, fr, fd, info=fw, world0=5, max_steps=500, **kw)
        ops.nav_env_step_info(ns, a, no, nr, nd, nw, env0=5, max_steps=500, **kw)
        compare(t)
        assert same(host(fr), host(nr)) and np.array_equal(host(fd), host(nd)) and np.array_equal(host(fw), host(nw)), t
        assert not host(fd).any() and not host(nd).any(), t


def test_repeats_are_bit_identical_and_the_info_word_changes_nothing():
    kw, want = reference(SWEEP[3])
    (a, _), (b, _), (c, env_c) = (play_on_device(kw, want["actions"], emit_info=e) for e in (True, True, False))
    assert_tape_equals(b, a)
    assert_tape_equals(c, a)
    assert a["info"].any() and "info" not in c and env_c.info is None


def test_the_env_owns_its_outputs_by_default():
    from ddrl4nav_amd.env import FleetNavEnv, make_device_env
    kw, want = reference(SWEEP[2])
    env = make_device_env({"env_name": "DeviceNavFleet-v0", "env_num": kw["n_worlds"], "agent_num_per_env": kw["n_robots"],
                           "env_seed": kw["seed"], "env_obstacles": 10, "env_peds": 0, "env_max_steps": 15, "env_info": True},
                          env0=kw["world0"])
    assert isinstance(env, FleetNavEnv) and env.state_shapes == SHAPES and env.N == 10 and env.n_envs == 10 and env.world0 == 1000
    out = env.reset()
    assert all(o is e for o, e in zip(out, env.obs)) and all(same(host(o), f) for o, f in zip(out, want["first"]))
    for t in range(10):
        o, r, d = env.step(dev(want["actions"][t]))
        assert all(x is e for x, e in zip(o, env.obs)) and r.dtype == torch.float32 and d.dtype == torch.uint8
    assert same(host(o[0]), want["laser"][9]) and same(host(o[2]), want["image"][9]) and np.array_equal(host(env.state), want["state"][9])
    assert np.array_equal(host(env.info), want["info"][9])


def test_masked_reset_is_per_world():
    """Only the worlds with a non-zero mask byte restart (all counters zero, the first observations of their rows rendered); the others
    keep their state and their rows of the observation, whatever those hold."""
    from ddrl4nav_amd.env import FleetNavEnv
    nw, nr = 5, 3
    kw = dict(seed=9, world0=2, n_obstacles=4, n_peds=3, max_steps=50)
    model, env = F.FleetEnvRef(nw, nr, **kw), FleetNavEnv(nw, nr, device="cuda", **kw)
    model.reset()
    env.reset()
    rng = np.random.RandomState(4)
    for t in range(12):
        a = rng.uniform(-1, 1, (nw * nr, 2)).astype(np.float32)
        model.step(a)
        env.step(dev(a))
    mask = np.array([0, 3, 0, 1, 255], np.uint8)
    rows = np.repeat(mask != 0, nr)
    before = model.state.copy()
    want = model.reset(mask)
    bufs = filled(1, nw * nr)
    got = env.reset(mask=dev(mask), obs_out=[b[0] for b in bufs])
    torch.cuda.synchronize()
    assert np.array_equal(host(env.state), model.state) and np.array_equal(model.state[[0, 2]], before[[0, 2]])
    assert (model.state[[1, 3, 4], F.EVENTS] == 1 + 4 + 2 * nr + 3).all()
    for g, w in zip(got, want):
        assert same(host(g)[rows], w[rows]) and is_fill(g[~torch.from_numpy(rows).cuda()])
    with pytest.raises(AssertionError):
        env.reset(mask=dev(np.ones(nw * nr, np.uint8)))                 # a byte per world, not per row
    a = rng.uniform(-1, 1, (nw * nr, 2)).astype(np.float32)             # and the episodes go on for all five worlds
    o, r, d = model.step(a)
    go, gr, gd = env.step(dev(a))
    assert np.array_equal(host(env.state), model.state) and all(same(host(x), y) for x, y in zip(go, o)) and same(host(gr), r)


def test_state_dict_resumes_bit_identically():
    from ddrl4nav_amd.env import FleetNavEnv
    kw, want = reference(SWEEP[3])
    _, env = play_on_device(kw, want["actions"][:20])
    sd = env.state_dict()
    assert not sd["state"].is_cuda and sd["n_robots"] == 3 and sd["n_worlds"] == 17 and sd["max_steps"] == 15
    got, _ = play_on_device(kw, want["actions"][20:], start=sd)         # a resumed env renders nothing before its first step: play_env
    assert_tape_equals(got, tape_from(want, 20))
    with pytest.raises(ValueError):
        FleetNavEnv(device="cuda", **dict(kw, n_robots=2)).load_state_dict(sd)
    with pytest.raises(ValueError):
        FleetNavEnv(device="cuda", **dict(kw, max_steps=16)).load_state_dict(sd)


def step_both(model, env, actions):
    """One step of the model and of the device env; everything compared.  -> done."""
    o, r, d = model.step(actions)
    go, gr, gd = env.step(dev(actions))
    assert np.array_equal(host(env.state), model.state), np.nonzero(host(env.state) != model.state)
    assert all(same(host(x), y) for x, y in zip(go, o)) and same(host(gr), r) and np.array_equal(host(gd), d)
    assert np.array_equal(host(env.info), model.info)
    return d


@pytest.mark.parametrize("nr,pops", [(4, (10, 5)), (3, (3, 2)), (1, (0, 0))])
def test_a_hostile_state_is_sanitised(nr, pops):
    """A state of random int32 words (and the extremes): the outputs equal the model's after sanitize(), nothing outside the env's rows
    is written, and the stored state is a sanitised one."""
    from ddrl4nav_amd.env import FleetNavEnv
    nw = 37
    kw = dict(seed=6, n_obstacles=pops[0], n_peds=pops[1], max_steps=40, world0=77)
    rng = np.random.RandomState(pops[0] + 1)
    words = rng.randint(-2 ** 31, 2 ** 31, size=(nw, 96), dtype=np.int64).astype(np.int32)
    words[0], words[1], words[2] = np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1
    for r in range(nr):                                                 # some worlds go on with their episodes
        words[3:20, 10 * r + F.STEPS] = rng.randint(0, 30, 17)
        words[3:20, 10 * r + F.X:10 * r + F.Y + 1] = rng.randint(-1500, 1500, (17, 2))
    model = F.FleetEnvRef(nw, nr, **kw)
    want = record(model, 2, first_state=words, actions=rng.uniform(-1, 1, (2, nw * nr, 2)).astype(np.float32))
    assert_tape_equals(play_env(FleetNavEnv(nw, nr, device="cuda", emit_info=True, **kw), want["actions"], start=words), want)
    assert 0 < want["done"][0].sum() < nw * nr
    kept = model.state.copy()
    model.sanitize()
    assert np.array_equal(model.state, kept)


def test_four_robots_on_one_point_respawn_one_after_the_other():
    """A sanitised state built by hand, 6 worlds: all four robots stand on one point, so all of them collide with each other (kind 3,
    nothing else claims it) and respawn in index order, each clear of the ones placed before it."""
    from ddrl4nav_amd.env import FleetNavEnv
    nw, nr = 6, 4
    kw = dict(seed=12, n_obstacles=10, n_peds=5, max_steps=50, world0=5)
    model, env = F.FleetEnvRef(nw, nr, **kw), FleetNavEnv(nw, nr, device="cuda", emit_info=True, **kw)
    model.reset()
    for w in range(nw):
        spot = model.state[w, 0:2].copy()                               # robot 0's start: clear of every obstacle and pedestrian
        for r in range(nr):
            model.state[w, 10 * r:10 * r + 2] = spot
    before = model.state.copy()
    model.sanitize()
    assert np.array_equal(model.state, before)
    env.state.copy_(dev(model.state))
    d = step_both(model, env, np.zeros((nw * nr, 2), np.float32))
    assert d.all() and (S.unpack_info(model.info)["collision"] == 3).all()
    xy = model.state[:, :40].reshape(nw, 4, 10)[:, :, :2].astype(np.int64)
    for a in range(4):
        for b in range(a + 1, 4):
            assert (((xy[:, a] - xy[:, b]) ** 2).sum(axis=1) >= F.CLEAR ** 2).all()
    step_both(model, env, np.full((nw * nr, 2), 0.5, np.float32))


def test_a_crowded_grid_makes_the_start_scan_advance():
    """A sanitised state built by hand, 8 worlds: obstacles on the centres of cells 0..9, pedestrians on 10..14, robots 2 and 3 on 15 and
    16, robots 0 and 1 together on cell 17 -- they collide and respawn with 17 (then 18) of the 25 cells blocked, so their start scans
    walk over several blocked cells."""
    from ddrl4nav_amd.env import FleetNavEnv
    nw, nr = 8, 4
    kw = dict(seed=3, n_obstacles=10, n_peds=5, max_steps=50, world0=40)
    model, env = F.FleetEnvRef(nw, nr, **kw), FleetNavEnv(nw, nr, device="cuda", emit_info=True, **kw)
    model.reset()
    centre = lambda cell: ((cell % 5 - 2) * R.CELL, (cell // 5 - 2) * R.CELL)
    for k in range(10):
        model.state[:, F.OBS0 + 3 * k:F.OBS0 + 3 * k + 3] = centre(k) + (100,)
    for j in range(5):
        model.state[:, F.PED0 + 4 * j:F.PED0 + 4 * j + 4] = centre(10 + j) + (960 * j % 3840, 8)
    for r, cell in enumerate((17, 17, 15, 16)):
        model.state[:, 10 * r:10 * r + 9] = centre(cell) + (0, 0, 0) + centre(24) + (700, 0)
    before = model.state.copy()
    model.sanitize()
    assert np.array_equal(model.state, before)
    env.state.copy_(dev(model.state))
    d = step_both(model, env, np.zeros((nw * nr, 2), np.float32)).reshape(nw, nr)
    assert d[:, :2].all() and not d[:, 2:].any()
    print("start scans went", model.scan_cells[0].reshape(nw, nr)[:, :2].ravel(), "goal scans", model.scan_cells[1].reshape(nw, nr)[:, :2].ravel())
    assert model.scan_cells[0].max() >= 3 and (model.scan_cells[0] >= 2).sum() >= 3 and model.scan_cells[1].max() >= 1


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from ddrl4nav_amd import ops
    from ddrl4nav_amd._lib import DdrlError
    from ddrl4nav_amd.env import FleetNavEnv
    env = FleetNavEnv(2, 2, device="cuda")
    flat = torch.zeros(4 * 960 + 16, dtype=torch.float32, device="cuda")
    with pytest.raises(AssertionError):
        env.reset(obs_out=[flat[1:1 + 4 * 960].view(4, 1, 960), env.obs[1], env.obs[2]])     # a laser base that is not 16-byte aligned
    env.reset(obs_out=[flat[4:4 + 4 * 960].view(4, 1, 960), env.obs[1], env.obs[2]])
    with pytest.raises(AssertionError):
        env.step(torch.zeros((4, 2), dtype=torch.float64, device="cuda"))
    with pytest.raises(AssertionError):
        env.step(torch.zeros((2, 2), dtype=torch.float32, device="cuda"))                    # a row per world is too few
    with pytest.raises(AssertionError):
        env.reset(obs_out=[env.obs[0], env.obs[1], torch.zeros((2, 3, 48, 48), device="cuda")])
    with pytest.raises(AssertionError):
        ops.fleet_env_reset(env.state, 5, env.obs)
    with pytest.raises(DdrlError):                                       # the reward inside the image
        ops.fleet_env_step(env.state, 2, torch.zeros((4, 2), device="cuda"), env.obs, env.obs[2].view(-1)[:4], env.done)
    with pytest.raises(DdrlError):
        ops.fleet_env_step(env.state, 2, torch.zeros((4, 2), device="cuda"), env.obs, env.reward, env.done, n_peds=6)


# ---- 2. the navigation status: one row per robot ----------------------------------------------------------------------------------------------
def test_nav_status_counts_the_other_robot_collisions():
    """NavStatus fed the DEVICE's info words of the coverage tape equals NavStatusRef in every per-row tensor; the fourth ring fills;
    other_robot_collision_rate() and summary() are the model's."""
    from ddrl4nav_amd.agent import NavStatus
    kw, tape = reference(TAPE)
    infos = play_on_device(kw, tape["actions"])[0]["info"]
    assert np.array_equal(infos, tape["info"])
    st, want = NavStatus(24, "cuda"), S.NavStatusRef(24)
    st.update(dev(infos))
    want.update(infos)
    assert_status_equals(st, want)
    assert host(st.coll_robot_num).sum() > 0
    rate, wanted = st.other_robot_collision_rate(), F.other_robot_collision_rate(want)
    print("other-robot collision rate:", rate, wanted)
    assert isinstance(rate, float) and wanted > 0 and close_to([rate], [wanted])
    summary, model = st.summary(), want.summary()
    assert tuple(summary) == S.SUMMARY_KEYS and close_to([summary[k] for k in S.SUMMARY_KEYS], [model[k] for k in S.SUMMARY_KEYS])


# ---- 3. the closed loop -----------------------------------------------------------------------------------------------------------------------
NW, NR, T = 2, 2, 8
N = NW * NR
ENV_KW = dict(seed=31, n_obstacles=10, n_peds=5, max_steps=5)           # every robot is done every fifth step at the latest


def test_closed_loop_equals_the_host_driven_rollout():
    """arena_harness.closed_loop on a FleetNavEnv, StateRollout(n_envs=env.N), the navigation status tracked: collect_states() with
    in-pool rendering against the host model through put_states, two rollouts with carry_over() between them."""
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.env import FleetNavEnv
    from ddrl4nav_amd.runner.device_loop import collect_states
    env = FleetNavEnv(NW, NR, device="cuda", emit_info=True, **ENV_KW)
    assert env.N == N == 4 and N * T == 32
    ra = StateRollout(make_net(N * T), env.N, SHAPES, horizon=T, track_returns=True, track_nav_status=True)
    with pytest.raises(ValueError):
        collect_states(ra, FleetNavEnv(NW, NR + 1, device="cuda", emit_info=True))            # 6 rows against a rollout of 4
    with pytest.raises(ValueError, match="emit_info"):
        collect_states(ra, FleetNavEnv(NW, NR, device="cuda"))
    out = closed_loop(env, F.FleetEnvRef(NW, NR, **ENV_KW), T, track_nav_status=True)
    assert out.dones[:T].any() and out.dones[T:].any() and out.dones.sum() >= 3 * N
    assert close_to([out.ra.nav_status.other_robot_collision_rate()], [F.other_robot_collision_rate(out.status)])


def test_train_states_runs_three_updates_on_a_fleet():
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.env import FleetNavEnv
    from ddrl4nav_amd.runner.device_loop import train_states
    net = make_net(N * T, seed=2)
    net.training_iter_time = 2
    env = FleetNavEnv(NW, NR, device="cuda", seed=4, max_steps=6)
    ro = StateRollout(net, env.N, SHAPES, horizon=T, track_returns=True)
    start = net.params.clone()
    out = list(train_states(net, env, ro, 3))
    assert len(out) == 3 and ro.rollouts == 3 and not torch.equal(net.params, start)
    for losses, mean_return in out:
        assert all(np.isfinite(losses[k]) for k in LOSS_KEYS)
    assert -16.5 <= out[-1][1] <= 16.5
