"""Host side of the multi-robot navigation env (tests/fleet_env_ref.py, the rule book of csrc/fleetenv.hip): the model anchored to
tests/nav_env_ref.py at one robot per world, its self-checks, the event coverage of the tape the GPU test replays, the header against the
binding table, the refusals of FleetNavEnv, make_device_env, the ops wrappers and the C ABI, and NavStatusRef fed the tape's info words.
No GPU."""
import functools
import itertools
import math

import numpy as np
import pytest

import fleet_env_ref as F
import nav_env_ref as R
import nav_status_ref as S
from arena_abi import BASE, caller, common_refusals, header_declares, overlaps, refused, sizes

NEW = ("ddrl_op_fleet_env_state_ints", "ddrl_op_fleet_env_reset", "ddrl_op_fleet_env_step")


@functools.lru_cache(maxsize=None)
def tape():
    return F.coverage_run()


# ---- 1. the anchor: a fleet of one robot is the navigation env --------------------------------------------------------------------------
def test_one_robot_per_world_is_the_nav_rule_book():
    """R = 1, 8 worlds, 10 obstacles, 5 pedestrians: the reset and every observation equal NavEnvRef's bit for bit, and so does every step
    in which no robot finishes -- every mapped state word, the reward and the event counter, pedestrian turns and their draws included.
    (A finished robot respawns alone here and draws a whole new episode there: from such a step on the nav model is re-seeded with the
    fleet's state.)"""
    n = 8
    fleet, nav = F.FleetEnvRef(n, 1, seed=3, max_steps=10 ** 6), R.NavEnvRef(n, seed=3, max_steps=10 ** 6)
    for a, b in zip(fleet.reset(), nav.reset()):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(F.nav_state(fleet.state), nav.state) and (fleet.state[:, F.EVENTS] == 3 + 10 + 5).all()
    rng = np.random.RandomState(1)
    compared = turns = 0
    for t in range(300):
        a = np.stack([rng.uniform(0.0, 0.6, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)
        nav.state[:] = F.nav_state(fleet.state)
        of, rf, df = fleet.step(a)
        on, rn, dn = nav.step(a)
        keep = (df == 0) & (dn == 0)
        assert np.array_equal(df, dn) and np.array_equal(rf.view(np.int32), rn.view(np.int32))
        assert np.array_equal(F.nav_state(fleet.state)[keep], nav.state[keep])
        assert np.array_equal(fleet.events["ped_turn"], nav.events["ped_turn"])
        for x, y in zip(of, on):
            assert np.array_equal(x[keep].view(np.int32), y[keep].view(np.int32))
        compared += int(keep.sum())
        turns += int(nav.events["ped_turn"][keep].sum())
    print("steps compared:", compared, "pedestrian turns among them:", turns)
    assert compared >= 200 and turns >= 10


# ---- 2. the model's self-checks -----------------------------------------------------------------------------------------------------------
def _far(ax, ay, bx, by):
    return ((ax - bx) ** 2 + (ay - by) ** 2 >= F.CLEAR ** 2).all()


def _check_spawn(m, world, r):
    """Robot r of `world` has just been placed: clear of every obstacle centre, pedestrian and other robot; its goal clear of every
    obstacle centre and in another cell; a fresh episode."""
    s = m.state[world].astype(np.int64)
    rob = s[:40].reshape(4, 10)
    o = s[F.OBS0:F.OBS0 + 3 * m.n_obstacles].reshape(-1, 3)
    p = s[F.PED0:F.PED0 + 4 * m.n_peds].reshape(-1, 4)
    x, y, gx, gy = rob[r, F.X], rob[r, F.Y], rob[r, F.GX], rob[r, F.GY]
    others = rob[[q for q in range(m.R) if q != r]]
    assert _far(x, y, o[:, 0], o[:, 1]) and _far(x, y, p[:, 0], p[:, 1]) and _far(x, y, others[:, F.X], others[:, F.Y])
    assert _far(gx, gy, o[:, 0], o[:, 1])
    assert x % R.CELL == 0 and y % R.CELL == 0 and max(abs(x), abs(y)) <= 2 * R.CELL                  # a cell centre
    assert max(abs(gx - x), abs(gy - y)) > 128                                                         # not the start cell's goal
    assert rob[r, F.V] == rob[r, F.W] == rob[r, F.STEPS] == 0
    assert rob[r, F.DPREV] == math.isqrt(int((gx - x) ** 2 + (gy - y) ** 2)) > R.GOAL_TOL


def test_model_invariants_over_seeded_play():
    """sanitize() is a no-op along a rule-made trajectory, every reset and every respawn is clear, the observation is a pure function of
    the state with exact values, unused words stay zero, and the discriminants stay far inside int64."""
    nw, nr, steps = 5, 3, 120
    m = F.FleetEnvRef(nw, nr, seed=5, max_steps=40)
    rng = np.random.RandomState(11)
    obs = m.reset()
    assert (m.state[:, F.EVENTS] == 1 + 10 + 2 * nr + 5).all()
    for w, r in itertools.product(range(nw), range(nr)):
        _check_spawn(m, w, r)
    respawns = 0
    for t in range(steps):
        a = np.stack([rng.uniform(0.3, 1.0, m.N), rng.uniform(-1.0, 1.0, m.N)], axis=1).astype(np.float32)
        a[0::2] = R.steering_actions(obs[1])[0::2]
        before_events = m.state[:, F.EVENTS].copy()
        obs, reward, done = m.step(a)
        kept = m.state.copy()
        m.sanitize()
        assert np.array_equal(m.state, kept)
        laser, vector, image = obs
        assert laser.shape == (m.N, 1, 960) and vector.shape == (m.N, 5) and image.shape == (m.N, 3, 48, 48)
        assert all(x.dtype == np.float32 for x in obs) and reward.dtype == np.float32 and done.dtype == np.uint8
        assert (laser >= 0).all() and (laser <= 6.0).all() and np.array_equal(laser * 256, np.round(laser * 256))
        assert np.isin(image[:, 0], (0.0, 1.0)).all() and (np.abs(image[:, 1:]) <= 1.0).all()
        assert np.array_equal(reward * 256, np.round(reward * 256)) and (np.abs(reward) <= 15.5).all()
        for x, y in zip(obs, m.observe()):
            assert np.array_equal(x, y)
        fin = done.reshape(nw, nr) != 0
        turns = m.events["ped_turn"]
        assert np.array_equal(m.state[:, F.EVENTS], before_events + turns + 2 * fin.sum(axis=1))        # two draws a respawn
        for w, r in zip(*np.nonzero(fin)):
            _check_spawn(m, w, r)                                       # a later respawn of the step keeps clear of it in turn
            respawns += 1
        rob = m.state[:, :40].reshape(nw, 4, 10)
        assert (rob[:, nr:] == 0).all() and (rob[:, :, 9] == 0).all() and (m.state[:, F.USED:] == 0).all()
        assert ((rob[:, :nr, F.STEPS] >= 0) & (rob[:, :nr, F.STEPS] < m.max_steps)).all()
        assert np.array_equal(S.unpack_info(m.info)["done"], done)
    assert respawns >= 10
    print("largest discriminant: 2^%.1f" % math.log2(m.max_disc))
    assert 0 < m.max_disc < 2 ** 55


def test_later_respawns_see_the_earlier_ones():
    """Four robots finished on one point: each respawn is clear of the robots placed before it in the same step, and of the ones that
    still wait at the old point."""
    m = F.FleetEnvRef(1, 4, seed=2, n_obstacles=0, n_peds=0, max_steps=50)
    m.reset()
    for r in range(4):
        m.state[0, 10 * r + F.X], m.state[0, 10 * r + F.Y] = 100, -100
    _, reward, done = m.step(np.zeros((4, 2), np.float32))
    assert done.tolist() == [1, 1, 1, 1] and (S.unpack_info(m.info)["collision"] == 3).all() and (reward < 0).all()
    xy = m.state[0, :40].reshape(4, 10)[:, :2].astype(np.int64)
    for a, b in itertools.combinations(range(4), 2):
        assert ((xy[a] - xy[b]) ** 2).sum() >= F.CLEAR ** 2
    assert m.state[0, F.EVENTS] == 1 + 8 + 8


def test_scans_terminate_on_random_sanitised_states():
    """1,000 random sanitised states with the full population, every robot finished at once: each scan finds a cell (the model asserts it
    instead of looping), and the respawned robots are clear."""
    nw = 1000
    m = F.FleetEnvRef(nw, 4, seed=9, max_steps=1, ranges=False)         # every robot is done after one step: 8 scans a world
    rng = np.random.RandomState(3)
    m.state[:] = rng.randint(-2 ** 31, 2 ** 31, size=(nw, 96), dtype=np.int64).astype(np.int32)
    m.state[: nw // 2, :F.EVENTS] = rng.randint(-2560, 2561, size=(nw // 2, F.EVENTS))    # half of them with every circle inside the grid
    m.state[: nw // 4, F.OBS0:F.EVENTS] = (rng.randint(-2, 3, size=(nw // 4, 50)) * R.CELL)   # a quarter with circles ON cell centres
    m.state[:, [10 * r + F.STEPS for r in range(4)]] = 0
    _, _, done = m.step(rng.uniform(-1, 1, (m.N, 2)).astype(np.float32))
    assert done.all()
    assert m.events["start_advanced"].sum() > 100 and m.events["goal_advanced"].sum() > 100
    print("longest scans:", m.scan_cells.max(axis=1))
    assert m.scan_cells.max() < F.CELLS and m.scan_cells[0].max() >= 5
    for w, r in itertools.product(range(0, nw, 7), range(4)):
        _check_spawn(m, w, r)


def test_unused_slots_stay_zero_and_populations_shape_the_draws():
    for nr, n_obs, n_peds in ((1, 0, 0), (4, 10, 0), (2, 0, 5), (3, 3, 2)):
        m = F.FleetEnvRef(3, nr, seed=2, n_obstacles=n_obs, n_peds=n_peds, max_steps=9, ranges=False)
        m.reset()
        assert (m.state[:, F.EVENTS] == 1 + n_obs + 2 * nr + n_peds).all()
        rng = np.random.RandomState(1)
        for t in range(20):
            obs, _, _ = m.step(rng.uniform(-1, 1, (m.N, 2)).astype(np.float32))
            assert (m.state[:, 10 * nr:F.OBS0] == 0).all() and (m.state[:, F.OBS0 + 3 * n_obs:F.PED0] == 0).all()
            assert (m.state[:, F.PED0 + 4 * n_peds:F.EVENTS] == 0).all() and (m.state[:, F.USED:] == 0).all()
            if n_peds == 0 and nr == 1:
                assert not obs[2].any()


def test_a_shard_plays_the_worlds_of_the_single_process():
    nw, a, b, nr = 5, 1, 4, 2
    kw = dict(seed=21, max_steps=30, ranges=False)
    whole, part = F.FleetEnvRef(nw, nr, **kw), F.FleetEnvRef(b - a, nr, world0=a, **kw)
    for x, y in zip(whole.reset(), part.reset()):
        assert np.array_equal(x[a * nr:b * nr], y)
    rng = np.random.RandomState(2)
    for t in range(60):
        act = np.stack([rng.uniform(0.3, 1.0, nw * nr), rng.uniform(-1.0, 1.0, nw * nr)], axis=1).astype(np.float32)
        ow, rw, dw = whole.step(act)
        op, rp, dp = part.step(act[a * nr:b * nr])
        assert np.array_equal(whole.state[a:b], part.state) and np.array_equal(rw[a * nr:b * nr], rp) and np.array_equal(dw[a * nr:b * nr], dp)
        assert np.array_equal(whole.info[a * nr:b * nr], part.info)


def test_robots_show_in_each_others_laser_and_map():
    """Two robots 200 ticks apart, nothing else: robot 0 looks at robot 1 and sees it 136 ticks ahead (200 less the radius 64) and in the
    map cells straight ahead with robot 1's velocity in robot 0's frame; a pedestrian on the same spot covers it."""
    m = F.FleetEnvRef(1, 2, n_obstacles=0, n_peds=1)
    m.reset()
    m.state[0, 0:9] = [0, 0, 0, 0, 0, 1000, 0, 1000, 0]
    m.state[0, 10:19] = [200, 0, 960, 16, 0, 1000, 0, 800, 0]           # heading +90 degrees, v = 16
    m.state[0, F.PED0:F.PED0 + 4] = [-2000, 0, 0, 8]
    laser, vector, image = m.observe()
    assert laser[0, 0, 0] == 136 / 256 and laser[1, 0, 240] == 136 / 256     # robot 1 sees robot 0 on its left... 90 degrees = beam 240
    assert image[0, 0, 20, 23] == 1.0 and image[0, 1, 20, 23] == 0.0 and image[0, 2, 20, 23] == 16 / 32   # 200 ahead: row 20; moving left
    assert image[0, 0].sum() < 20
    m.state[0, F.PED0:F.PED0 + 2] = [200, 0]                             # the pedestrian on robot 1: it wins the shared cells
    _, _, image2 = m.observe()
    assert image2[0, 2, 20, 23] == 0.0 and image2[0, 1, 20, 23] == 8 / 32 and image2[0, 0].sum() >= image[0, 0].sum()


# ---- 3. the coverage tape -------------------------------------------------------------------------------------------------------------------
TAPE_COUNTS = {"ped_turn": 119, "wall_hit": 22, "obstacle_hit": 44, "ped_hit": 11, "robot_hit": 20, "goal": 31, "trunc": 3,
               "start_advanced": 68, "goal_advanced": 58}


def test_the_coverage_tape_holds_every_event_class():
    """The tape the GPU test replays: 6 worlds x 4 robots, 300 steps, seed 7, 10 obstacles, 5 pedestrians, max_steps = 120; even rows
    steer to the goal, odd rows act at random.  The counts are this model's own; every class occurs at least three times."""
    assert F.COVERAGE == dict(n_worlds=6, n_robots=4, seed=7, n_obstacles=10, n_peds=5, max_steps=120) and F.COVERAGE_STEPS == 300
    counts, actions, first, trace = tape()
    print(counts)
    assert actions.shape == (300, 24, 2) and len(trace) == 300
    assert (actions[:, 1::2, 0] >= 0.3).all() and np.isin(actions[:, 0::2, 0], np.float32([1.0, 0.2])).all()
    for k in F.EVENT_NAMES:
        assert counts[k] >= 3, (k, counts)
    assert counts == TAPE_COUNTS
    rewards = np.stack([step[2] for step in trace])
    assert (rewards > 14).any() and (rewards < -14).any()
    kinds = S.unpack_info(np.stack([step[4] for step in trace]))["collision"]
    assert all((kinds == k).sum() >= 3 for k in (1, 2, 3))              # a robot-robot collision that nothing else claims


def test_nav_status_ref_counts_the_other_robot_collisions():
    """NavStatusRef fed the tape's info words, one status row per robot: the fourth ring fills, and the rate is the plain formula."""
    _, _, _, trace = tape()
    words = np.stack([step[4] for step in trace])
    status = S.NavStatusRef(24)
    status.update(words)
    assert status.coll_robot_num.sum() > 0
    per_row = np.zeros(24)
    for row in range(24):                                               # spelled out, row by row
        episodes = int(S.unpack_info(words[:, row])["done"].sum())
        assert episodes == status.episode_num[row] < 100
        per_row[row] = float(status.coll_robot_num[:, row].sum()) / min(max(episodes + 1, 1), 100)
    rate = F.other_robot_collision_rate(status)
    print("other-robot collision rate of the tape:", rate)
    assert 0 < rate < 1 and abs(rate - per_row.mean()) <= 1e-12               # 24 float64 terms of at most 1
    # every finished episode's kind-3 end is in the ring: the windows are not full, so nothing has been overwritten but the running slot
    f = S.unpack_info(words)
    ended_by_robot = ((f["collision"] == 3) & (f["done"] == 1)).sum(axis=0)
    assert np.array_equal(status.coll_robot_num.sum(axis=0).astype(np.int64), ended_by_robot)
    summary = status.summary()
    assert set(summary) == set(S.SUMMARY_KEYS)                          # the 11 keys do not change


# ---- 4. header, binding, wrappers -------------------------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_binds():
    from ddrl4nav_amd import ops
    _, lib = header_declares(NEW, [0, 12, 16])
    assert lib.ddrl_op_fleet_env_state_ints() == F.STATE_INTS == ops.fleet_env_state_ints() == 96
    assert ops.FLEET_ENV_MAX_ROBOTS == F.MAX_ROBOTS == 4
    assert ops.nav_env_state_ints() == 64 and ops.NAV_STATUS_SUMMARY == 22 and ops.ENV_GAMES == {"pong": 0, "catch": 1}
    assert all(hasattr(ops, k) for k in ("fleet_env_state_ints", "fleet_env_reset", "fleet_env_step"))


def test_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses: every refusal below is decided before the first HIP call.  The fabricated call:
    4 worlds x 2 robots = 8 rows."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    size, obs = sizes("ddrl_op_fleet_env_reset"), ("st", "la", "ve", "im")
    shapes = [dict(nw=0), dict(nr=0), dict(nr=5), dict(e0=2 ** 32 - 3), dict(nw=2 ** 30, nr=2)]
    bad = [{p: None} for p in obs] + shapes + [dict(nw=-4), dict(nr=-1), dict(e0=-1), dict(e0=2 ** 32), dict(nobs=-1), dict(nobs=11),
                                               dict(nped=-1), dict(nped=6), dict(nw=2 ** 29 + 1, nr=4), dict(nw=2 ** 31 - 1, nr=3)]
    bad += [dict(st=BASE["st"] + 4), dict(la=BASE["la"] + 8), dict(la=BASE["la"] + 4), dict(im=BASE["im"] + 1), dict(im=BASE["im"] + 8),
            dict(ve=BASE["ve"] + 2)]
    bad += overlaps(obs, size)
    bad += [{"mask": BASE[p]} for p in obs] + [{"mask": BASE[p] + size[p] - 1} for p in obs]
    bad += [{"mask": BASE["st"] - 3}]                                   # a byte per world, ending inside the state
    refused(caller(lib, "ddrl_op_fleet_env_reset"), bad)
    step = caller(lib, "ddrl_op_fleet_env_step")
    shapes += [dict(nw=-1), dict(nr=-2), dict(nw=2 ** 31 - 1, nr=4)]
    refused(step, common_refusals("ddrl_op_fleet_env_step") + shapes)
    refused(step, common_refusals("ddrl_op_fleet_env_step", without=("info",)) + shapes, info=None)    # this entry may go without it



def test_fleet_nav_env_refuses_bad_arguments():
    from ddrl4nav_amd.env import FLEET_ENV_NAME, FleetNavEnv, make_device_env
    assert FleetNavEnv.state_shapes == [(1, 960), (5,), (3, 48, 48)] and FLEET_ENV_NAME == "DeviceNavFleet-v0"
    for args, kw in (((0, 2), {}), ((-2, 2), {}), ((4, 0), {}), ((4, 5), {}), ((4, -1), {}), ((2 ** 30, 2), {}),
                     ((4, 2), dict(n_obstacles=11)), ((4, 2), dict(n_obstacles=-1)), ((4, 2), dict(n_peds=6)), ((4, 2), dict(n_peds=-1)),
                     ((4, 2), dict(max_steps=0)), ((4, 2), dict(seed=-1)), ((4, 2), dict(seed=2 ** 32)), ((4, 2), dict(world0=-1)),
                     ((4, 2), dict(world0=2 ** 32 - 3))):
        with pytest.raises(ValueError):                                 # before anything is allocated: no GPU is needed to refuse
            FleetNavEnv(*args, **kw)
    fleet = {"env_name": "DeviceNavFleet-v0", "env_num": 4, "agent_num_per_env": 2}
    for cfg in ({"env_name": "DeviceNav-v1", "env_num": 4}, {"env_name": "DeviceNavFleet-v1", "env_num": 4, "agent_num_per_env": 2},
                {"env_name": "DeviceNavFleet-v0", "env_num": 4}, {"env_name": "DeviceNavFleet-v0", "agent_num_per_env": 2},
                dict(fleet, env_num=0), dict(fleet, agent_num_per_env=0), dict(fleet, agent_num_per_env=5), dict(fleet, env_obstacles=11),
                dict(fleet, env_peds=6), dict(fleet, env_max_steps=0), dict(fleet, env_seed=-1)):
        with pytest.raises(ValueError):
            make_device_env(cfg)
    with pytest.raises(ValueError, match="DeviceNavFleet-v0"):          # the unknown-name branch lists the new name too
        make_device_env({"env_name": "DeviceNav-v1", "env_num": 4})


def test_ops_wrappers_refuse_host_tensors():
    import torch
    from ddrl4nav_amd import ops
    st = torch.zeros((2, 96), dtype=torch.int32)
    obs = [torch.zeros((4,) + s) for s in ops.NAV_ENV_SHAPES]
    with pytest.raises(AssertionError):
        ops.fleet_env_reset(st, 2, obs)
    with pytest.raises(AssertionError):
        ops.fleet_env_step(st, 2, torch.zeros((4, 2)), obs, torch.zeros(4), torch.zeros(4, dtype=torch.uint8))


def test_nav_status_has_the_other_robot_rate_and_keeps_its_summary():
    from ddrl4nav_amd.agent import statistics
    assert callable(statistics.NavStatus.other_robot_collision_rate)
    assert statistics.NAV_SUMMARY_KEYS == S.SUMMARY_KEYS and len(statistics.NAV_SUMMARY_KEYS) == 11
    assert "stays zero" not in statistics.NavStatus.__doc__
