"""Host side of the pedestrian model "avoid" (tests/ped_avoid_ref.py is the rule book of rule 1 under it): the rule
book anchored to tests/nav_env_ref.py and tests/fleet_env_ref.py under "walk" and to itself at one robot, every branch of the rule counted
on fixed states, the two invariants, the scripted expert's quality among pedestrians that give way, the header against the binding
table, every argument check of the two new entry points (decided before HIP) and the wrappers' knobs.  No GPU."""
import functools
import itertools
import re

import numpy as np
import pytest

import fleet_env_ref as F
import nav_env_ref as R
import nav_expert_ref as E
import ped_avoid_ref as P
from arena_abi import caller, common_refusals, header_declares, refused
from arena_harness import bits

NEW = ("ddrl_op_nav_env_step_model", "ddrl_op_fleet_env_step_model")


@functools.lru_cache(maxsize=None)
def nav_tape(ped_model):
    return P.nav_coverage_run(ped_model, ranges=False)


@functools.lru_cache(maxsize=None)
def fleet_tape(ped_model):
    return P.fleet_coverage_run(ped_model, ranges=False)


# ---- 1. the rule book is anchored -------------------------------------------------------------------------------------------------------
def test_walk_is_nav_env_ref_on_its_coverage_tape():
    """NavEnvPedRef re-spells NavEnvRef.step: under "walk" every state word, reward, done and event count of the coverage tape is
    NavEnvRef's (the observation too, on the first 40 steps: it is a function of the state)."""
    counts, actions, first, trace = R.coverage_run()
    _, c2, a2, f2, t2, info, played, _ = nav_tape("walk")
    assert counts == c2 and np.array_equal(bits(actions), bits(a2))
    for t, (x, y) in enumerate(zip(trace, t2)):
        assert np.array_equal(x[0], y[0]), t
        assert np.array_equal(bits(x[2]), bits(y[2])) and np.array_equal(x[3], y[3]), t
    m = P.NavEnvPedRef(ped_model="walk", **R.COVERAGE)
    for o, f in zip(m.reset(), first):
        assert np.array_equal(bits(o), bits(f))
    for t in range(40):
        obs, _, _ = m.step(actions[t])
        assert all(np.array_equal(bits(o), bits(w)) for o, w in zip(obs, trace[t][1])), t


def test_walk_is_nav_info_env_ref_too():
    """The info words and the played states of the re-spelled step are tests/nav_status_ref.py's."""
    import nav_status_ref as S
    kw = dict(R.COVERAGE, max_steps=25)
    _, actions, _, _, info, played = S.play_info(S.NavInfoEnvRef(ranges=False, **kw), 120, np.random.RandomState(0))
    m = P.NavEnvPedRef(ped_model="walk", ranges=False, **kw)
    m.reset()
    for t in range(120):
        m.step(actions[t])
        assert np.array_equal(m.info, info[t]) and np.array_equal(m.played, played[t]), t
    assert (info & 16).any()


def test_walk_is_fleet_env_ref_on_its_coverage_tape():
    ref = F.FleetEnvRef(ranges=False, **F.COVERAGE)
    counts, actions, first, trace = F.play(ref, F.COVERAGE_STEPS, np.random.RandomState(0))
    _, c2, a2, f2, t2 = fleet_tape("walk")
    assert counts == c2 and np.array_equal(bits(actions), bits(a2))
    for t, (x, y) in enumerate(zip(trace, t2)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[4], y[4]), t
        assert np.array_equal(bits(x[2]), bits(y[2])) and np.array_equal(x[3], y[3]), t
        assert all(np.array_equal(bits(o), bits(w)) for o, w in zip(x[1][1:], y[1][1:])), t        # vector and map (no ranges cast)


def test_one_robot_per_world_is_the_nav_model_under_avoid():
    """R = 1, as tests/test_fleet_env_cpu.py anchors the two "walk" rule books: before every step the nav model takes the fleet's state;
    the played states (the state before any new episode or respawn), rewards, dones and info words are equal."""
    n = 8
    kw = dict(seed=3, n_obstacles=6, n_peds=5, max_steps=40)
    fleet = P.FleetEnvPedRef(n, 1, ped_model="avoid", ranges=False, **kw)
    nav = P.NavEnvPedRef(n, ped_model="avoid", ranges=False, **kw)
    fleet.reset()
    rng = np.random.RandomState(1)
    dones = 0
    for t in range(200):
        a = np.stack([rng.uniform(0.3, 1.0, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)
        nav.state[:] = F.nav_state(fleet.state)
        _, fr, fd = fleet.step(a)
        _, nr, nd = nav.step(a)
        assert np.array_equal(F.nav_state(fleet.played), nav.played), t
        assert np.array_equal(bits(fr), bits(nr)) and np.array_equal(fd, nd) and np.array_equal(fleet.info, nav.info), t
        assert np.array_equal(fleet.events["ped_turn"], nav.events["ped_turn"])
        dones += int(fd.sum())
    assert dones >= 10 and fleet.branches == nav.branches and sum(fleet.branches["rank%d" % r] for r in range(1, 7)) > 0


# ---- 2. every branch --------------------------------------------------------------------------------------------------------------------
def test_every_branch_is_taken():
    """The model's own counts, as constants: a rule change shows here first.  The coverage tapes miss "blocked" (and the nav tape rank
    6); the crafted states take each branch with pedestrian 0."""
    nav, fleet = nav_tape("avoid")[0], fleet_tape("avoid")[0]
    assert nav.branches == {"rank0": 11856, "rank1": 4, "rank2": 5, "rank3": 6, "rank4": 3, "rank5": 3, "rank6": 0, "static": 123,
                            "blocked": 0}, nav.branches
    assert fleet.branches == {"rank0": 8854, "rank1": 12, "rank2": 7, "rank3": 6, "rank4": 1, "rank5": 2, "rank6": 3, "static": 115,
                              "blocked": 0}, fleet.branches
    states = P.branch_states()
    assert P.first_ped_branch(states, **P.BRANCH_POPULATION).tolist() == list(range(len(P.BRANCHES)))
    m = P.NavEnvPedRef(len(states), ped_model="avoid", ranges=False, seed=2, max_steps=500, **P.BRANCH_POPULATION)
    m.state[:] = states
    m.step(np.zeros((len(states), 2), np.float32))
    assert m.branches == {"rank0": 15, "rank1": 4, "rank2": 1, "rank3": 5, "rank4": 3, "rank5": 2, "rank6": 3, "static": 1,
                          "blocked": 11}, m.branches
    assert all(m.branches[k] + nav.branches[k] > 0 for k in P.BRANCHES)
    assert nav_tape("avoid")[1]["ped_turn"] == nav.branches["static"] + nav.branches["blocked"]     # every draw of rule 1 is counted


def test_constants_and_products_fit():
    assert P.KEEP == 192 and P.D == 320 and P.OFFSETS.tolist() == [0, 320, -320, 640, -640, 960, -960]
    assert 2 * (2 * (R.ARENA_R + R.SPEED_MAX)) ** 2 < 2 ** 31               # |c - q|^2 with both inside +-(2560 + 24)
    assert P.KEEP < 300                                                     # placement and respawn put agents at least 300 apart
    with pytest.raises(ValueError):
        P.NavEnvPedRef(2, ped_model="flee")
    with pytest.raises(ValueError):
        P.FleetEnvPedRef(2, 2, ped_model=1)


# ---- 3. the invariants ------------------------------------------------------------------------------------------------------------------
def test_pedestrians_keep_their_distance_on_both_tapes():
    """From a reset no two pedestrians in use are ever nearer than KEEP, after every step; under "walk" they are."""
    worst = {}
    for name, tape, ped0, n in (("nav", nav_tape, R.PED0, 8), ("fleet", fleet_tape, F.PED0, 6)):
        for model in P.MODELS:
            trace = tape(model)[4]
            worst[name, model] = min(P.min_ped_distance2(s[0][:, ped0:ped0 + 20].reshape(n, 5, 4)) for s in trace)
    print(worst)
    assert worst["nav", "avoid"] >= P.KEEP ** 2 and worst["fleet", "avoid"] >= P.KEEP ** 2
    assert worst["nav", "walk"] < P.KEEP ** 2 and worst["fleet", "walk"] < P.KEEP ** 2


def head_on(ped_model, steps=60):
    m = P.NavEnvPedRef(1, n_obstacles=0, n_peds=1, max_steps=500, ped_model=ped_model, ranges=False)
    m.state[:] = P.head_on_state()
    hits, nearest = [], []
    for _ in range(steps):
        m.step(np.zeros((1, 2), np.float32))
        hits.append(int(m.events["ped_hit"][0]))
        s = m.played[0].astype(np.int64)
        nearest.append(int((s[R.PED0] - s[R.X]) ** 2 + (s[R.PED0 + 1] - s[R.Y]) ** 2))
    return hits, nearest


def test_a_robot_that_stands_still_is_not_hit():
    """A pedestrian walks head-on at a robot that never moves: "walk" runs it into the robot (collision kind 2, charged to the robot),
    "avoid" leads it around -- the distance never drops below KEEP, because only the robot's own move can bring it there."""
    hits, _ = head_on("walk")
    assert sum(hits) >= 1 and hits.index(1) == 16                           # the hit of step 17
    hits, nearest = head_on("avoid")
    assert sum(hits) == 0
    assert min(nearest) >= P.KEEP ** 2 and min(nearest) < 300 ** 2          # it did come by


# ---- 4. the expert among pedestrians that give way --------------------------------------------------------------------------------------
# Measured with these rules at N = 128, 500 steps, seed 3, max_steps = 300 (goals, obstacle hits, pedestrian hits, wall hits, truncations):
#   (10, 5)  walk 733 13 48 0 0  reach rate 0.923     avoid 756 14 12 0 0  reach rate 0.967
#   (3, 2)   walk 925  2 14 0 0  reach rate 0.983     avoid 919  2  3 0 0  reach rate 0.995
def test_expert_reaches_its_goals_under_avoid():
    totals, branches = P.expert_tape("avoid", 128, 500, 3, 10, 5, 300)
    rate = E.reach_rate(totals)
    print(totals, "reach rate %.3f" % rate, branches)
    assert totals["goal"] > 500
    assert rate >= 0.85, (totals, rate)                                     # tests/test_nav_expert_cpu.py's floor for "walk"
    assert all(branches[k] > 0 for k in P.BRANCHES), branches                # all seven ranks and "blocked" occur on this tape


# ---- 5. header, binding, argument checks ------------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_binds():
    from ddrl4nav_amd import _lib, ops
    text, _ = header_declares(NEW, [19, 20])                                # additive: the ABI version stays 3
    assert re.search(r"#define\s+DDRL_PED_WALK\s+0\b", text) and re.search(r"#define\s+DDRL_PED_AVOID\s+1\b", text)
    assert callable(ops.nav_env_step_model) and callable(ops.fleet_env_step_model)
    assert ops.NAV_PED_MODELS == P.MODELS and [ops.nav_ped_model(m) for m in P.MODELS] == [0, 1] == [ops.nav_ped_model(k) for k in (0, 1)]
    for bad in ("flee", "", 2, -1, None, 1.0, True):
        with pytest.raises(ValueError):
            ops.nav_ped_model(bad)
    # the entries that were there keep their signatures
    assert [len(_lib.SIGNATURES[n][1]) for n in ("ddrl_op_nav_env_step", "ddrl_op_nav_env_step_info", "ddrl_op_nav_env_step_final",
                                                 "ddrl_op_fleet_env_step", "ddrl_op_fleet_env_step_final")] == [14, 15, 18, 16, 19]


FINAL = ("fl", "fv", "fi")


def test_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses: every refusal is decided before the first HIP call.  What tests/
    test_truncation_cpu.py asks of the _final entries (arena_abi.common_refusals), through the new ones, then what is new: the pedestrian
    model, the terminal triple in part, the terminal triple without info; and all of it with fewer outputs."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    partial = [dict.fromkeys(part) for k in (1, 2) for part in itertools.combinations(FINAL, k)] + [dict(info=None)]
    for name, shapes in (("ddrl_op_nav_env_step_model", [dict(n=0), dict(n=-2)]),
                         ("ddrl_op_fleet_env_step_model", [dict(nw=0), dict(nw=-1), dict(nr=0), dict(nr=5), dict(nw=2 ** 30, nr=2)])):
        step = caller(lib, name)
        own = shapes + [dict(pm=2), dict(pm=-1), dict(pm=256), dict(pm=2 ** 31 - 1)]
        for pm in (0, 1):
            refused(step, common_refusals(name) + own + partial, pm=pm)
            refused(step, common_refusals(name, without=FINAL) + own, pm=pm, **dict.fromkeys(FINAL))           # info alone
            refused(step, common_refusals(name, without=("info",) + FINAL) + own, pm=pm, **dict.fromkeys(("info",) + FINAL))    # none


def test_ops_wrappers_refuse_host_tensors_and_bad_models():
    import torch
    from ddrl4nav_amd import ops
    obs = [torch.zeros((4,) + s) for s in ops.NAV_ENV_SHAPES]
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    with pytest.raises(AssertionError):
        ops.nav_env_step_model(i32(4, 64), torch.zeros((4, 2)), obs, torch.zeros(4), torch.zeros(4, dtype=torch.uint8), ped_model="avoid")
    with pytest.raises(AssertionError):
        ops.fleet_env_step_model(i32(2, 96), 2, torch.zeros((4, 2)), obs, torch.zeros(4), torch.zeros(4, dtype=torch.uint8),
                                 ped_model="avoid")


# ---- 6. the wrappers' knobs -------------------------------------------------------------------------------------------------------------
def test_env_constructors_refuse_a_bad_model():
    """Decided before anything is allocated: no device is needed."""
    from ddrl4nav_amd.env import DeviceNavEnv, FleetNavEnv
    for bad in ("flee", "", "Avoid", None, 1, 0):
        with pytest.raises(ValueError, match="ped_model"):
            DeviceNavEnv(4, device="cpu", ped_model=bad)
        with pytest.raises(ValueError, match="ped_model"):
            FleetNavEnv(2, 2, device="cpu", ped_model=bad)
    assert "ped_model" in DeviceNavEnv._PARAMS and "ped_model" in FleetNavEnv._PARAMS


def test_arena_config_kw_defaults_to_walk(monkeypatch):
    from ddrl4nav_amd.env import device_nav_env, fleet_nav_env, make_device_env
    assert device_nav_env.arena_config_kw({})["ped_model"] == "walk"
    assert device_nav_env.arena_config_kw({"env_ped_model": "avoid"})["ped_model"] == "avoid"
    seen = []
    monkeypatch.setattr(device_nav_env, "DeviceNavEnv", lambda *a, **k: seen.append(k) or "nav")
    monkeypatch.setattr(fleet_nav_env, "FleetNavEnv", lambda *a, **k: seen.append(k) or "fleet")
    assert make_device_env({"env_name": "DeviceNav-v0", "env_num": 4, "env_ped_model": "avoid"}) == "nav"
    assert make_device_env({"env_name": "DeviceNavFleet-v0", "env_num": 4, "agent_num_per_env": 2, "env_ped_model": "avoid"}) == "fleet"
    assert make_device_env({"env_name": "DeviceNav-v0", "env_num": 4}) == "nav"
    assert [k["ped_model"] for k in seen] == ["avoid", "avoid", "walk"]


def test_a_state_dict_without_the_key_loads_as_walk():
    """An env saved before there was a choice: its state_dict has no ped_model and is one of "walk" (host tensors: no device needed)."""
    import torch
    from ddrl4nav_amd.env import DeviceNavEnv, FleetNavEnv
    from ddrl4nav_amd.env.device_nav_env import NavArenaEnv
    for cls, words, params, rows in ((DeviceNavEnv, 64, dict(env0=5), dict(n_envs=3)),
                                     (FleetNavEnv, 96, dict(n_worlds=3, n_robots=2, world0=5), {})):
        common = dict(seed=1, n_obstacles=4, n_peds=2, max_steps=9)
        for model, ok in (("walk", True), ("avoid", False)):
            env = cls.__new__(cls)                                          # no allocation on a device: the checkpoint logic alone
            for k, v in dict(common, ped_model=model, **params).items():
                setattr(env, k, v)
            env.N = 3                                                       # DeviceNavEnv's n_envs
            env.state = torch.zeros((3, words), dtype=torch.int32)
            old = dict(common, state=torch.full((3, words), 7, dtype=torch.int32), **params, **rows)
            assert "ped_model" not in old and set(old) == set(cls._PARAMS) - {"ped_model"} | {"state"}
            if ok:
                env.load_state_dict(old)
                assert int(env.state.sum()) == 7 * 3 * words
            else:
                with pytest.raises(ValueError, match="ped_model"):
                    env.load_state_dict(old)
            sd = NavArenaEnv.state_dict(env)
            assert sd["ped_model"] == model
