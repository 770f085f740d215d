"""The pedestrian model "avoid" on the GPU (csrc/navcore.h nav_walk_peds_avoid in the step kernels of csrc/navenv.hip and
csrc/fleetenv.hip) against the integer rule book tests/ped_avoid_ref.py: every state word, lidar range, vector
entry, map cell, reward, done, info word and terminal observation after every step, bit for bit, through every form of both envs; the
"walk" model through the new entry points against the old ones; repeats, checkpoints and the closed loop.  Run with `-m gpu`."""
import functools

import numpy as np
import pytest

import fleet_env_ref as F
import nav_env_ref as R
import ped_avoid_ref as P
from arena_harness import HOSTILE, assert_tape_equals, closed_loop, is_fill, play_env, play_ops, record, tape_from

pytestmark = pytest.mark.gpu

FORMS = {"plain": {}, "info": dict(emit_info=True), "final": dict(emit_final_obs=True)}


# ---- the rule book's tapes: computed once, never modified -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nav_reference(case):
    """case = (N, n_obstacles, n_peds, env0, max_steps, steps, seed)."""
    n, n_obs, n_peds, env0, max_steps, steps, seed = case
    kw = dict(n_envs=n, seed=seed, n_obstacles=n_obs, n_peds=n_peds, max_steps=max_steps, env0=env0)
    hostile = {t: np.roll(HOSTILE, t, axis=0) for t in (7, 23)}
    return kw, record(P.NavEnvPedRef(ped_model="avoid", **kw), steps, np.random.RandomState(n + n_obs + n_peds), hostile=hostile)


@functools.lru_cache(maxsize=None)
def fleet_reference(case):
    """case = (n_worlds, R, n_obstacles, n_peds, world0, max_steps, steps, seed)."""
    nw, nr, n_obs, n_peds, world0, max_steps, steps, seed = case
    kw = dict(n_worlds=nw, n_robots=nr, seed=seed, n_obstacles=n_obs, n_peds=n_peds, max_steps=max_steps, world0=world0)
    return kw, record(P.FleetEnvPedRef(ped_model="avoid", **kw), steps, np.random.RandomState(nr))


# ---- 1. the navigation env under "avoid" ------------------------------------------------------------------------------------------------
TAPE = (8, 10, 5, 0, 120, 300, 7)                                       # the coverage populations: N = 8, 300 steps


def nav_env(kw, form, ped_model="avoid"):
    from ddrl4nav_amd.env import DeviceNavEnv
    return DeviceNavEnv(device="cuda", ped_model=ped_model, **FORMS[form], **kw)


def test_the_nav_tape_equals_the_rule_book_through_every_form():
    """All 64 state words, the 960 ranges, the vector, the map, the reward, the done, the info word and the truncated rows of final_obs
    after every step, bit for bit; and the three forms play one trajectory."""
    kw, want = nav_reference(TAPE)
    assert want["done"].sum() > 20 and len(want["final"]) >= 1 and (want["info"] >> 2 & 3 == 2).any()
    got = {form: play_env(nav_env(kw, form), want["actions"]) for form in FORMS}
    for form in FORMS:
        assert_tape_equals(got[form], want)
    assert "info" not in got["plain"] and "final" not in got["plain"] and "final" not in got["info"] and len(got["final"]["final"][0]) == 300
    assert_tape_equals(got["info"], got["plain"])
    assert_tape_equals(got["final"], got["info"])


SWEEP = [(n, n_obs, n_peds, 1000 + 7 * n_peds, 9, 40, 100 + n) for n in (1, 3) for n_peds in (0, 1, 2, 5) for n_obs in (0, 10)]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "N%d-obs%d-ped%d" % c[:3])
def test_nav_sweep_equals_the_rule_book(case):
    """No other pedestrian, no pedestrian, no obstacle, a non-zero env0, and max_steps = 9: respawn churn."""
    kw, want = nav_reference(case)
    assert want["done"].any() and want["final"]
    assert_tape_equals(play_env(nav_env(kw, "final"), want["actions"]), want)


def test_the_branch_states_equal_the_rule_book():
    """The crafted states of tests/test_ped_avoid_cpu.py -- every rank won, the static refusal, everything blocked -- after one step."""
    states = P.branch_states()
    kw = dict(n_envs=len(states), seed=2, max_steps=500, env0=3, **P.BRANCH_POPULATION)
    model = P.NavEnvPedRef(ped_model="avoid", **kw)
    want = record(model, 2, first_state=states, actions=np.zeros((2, len(states), 2), np.float32))
    assert all(model.branches[k] > 0 for k in P.BRANCHES)
    assert_tape_equals(play_env(nav_env(kw, "final"), want["actions"], start=states), want)


def test_the_head_on_pedestrian_walks_around_the_robot():
    """60 steps of a robot that stands still: the rule book's trajectory, no pedestrian hit; under "walk" the same state is hit."""
    kw = dict(n_envs=1, seed=0, n_obstacles=0, n_peds=1, max_steps=500)
    acts = np.zeros((60, 1, 2), np.float32)
    want = record(P.NavEnvPedRef(ped_model="avoid", **kw), 60, first_state=P.head_on_state(), actions=acts)
    got = play_env(nav_env(kw, "info"), acts, start=P.head_on_state())
    assert_tape_equals(got, want)
    assert not ((got["info"] >> 2) & 3).any() and not got["done"].any()
    walked = play_env(nav_env(kw, "info", ped_model="walk"), acts, start=P.head_on_state())
    assert (((walked["info"] >> 2) & 3) == 2).sum() >= 1


@pytest.mark.parametrize("pops", [(10, 5), (3, 2)])
def test_a_hostile_state_is_sanitised(pops):
    """A state of random int32 words (and the extremes): the outputs equal the model's after sanitize()."""
    n = 37
    kw = dict(n_envs=n, seed=6, n_obstacles=pops[0], n_peds=pops[1], max_steps=40, env0=77)
    rng = np.random.RandomState(pops[0] + 1)
    words = rng.randint(-2 ** 31, 2 ** 31, size=(n, 64), dtype=np.int64).astype(np.int32)
    words[0], words[1], words[2] = np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1
    words[3:20, R.STEPS] = rng.randint(0, 30, 17)
    words[3:20, R.X:R.Y + 1] = rng.randint(-1500, 1500, (17, 2))
    acts = rng.uniform(-1, 1, (2, n, 2)).astype(np.float32)
    want = record(P.NavEnvPedRef(ped_model="avoid", **kw), 2, first_state=words, actions=acts)
    assert_tape_equals(play_env(nav_env(kw, "final"), acts, start=words), want)
    assert 0 < want["done"][0].sum() < n


# ---- 2. the fleet under "avoid" ---------------------------------------------------------------------------------------------------------
def fleet_env(kw, form, ped_model="avoid"):
    from ddrl4nav_amd.env import FleetNavEnv
    return FleetNavEnv(device="cuda", ped_model=ped_model, **FORMS[form], **kw)


@pytest.mark.parametrize("nr", [1, 2, 3, 4])
def test_the_fleet_equals_the_rule_book(nr):
    """3 worlds, 150 steps, the info and the final form; the tape holds steps in which one robot finishes while the others go on."""
    kw, want = fleet_reference((3, nr, 10, 5, 11, 30, 150, 7))
    done = want["done"].reshape(150, 3, nr)
    assert want["final"] and done.any()
    if nr > 1:
        assert ((done.sum(axis=2) > 0) & (done.sum(axis=2) < nr)).any()
    for form in ("info", "final"):
        assert_tape_equals(play_env(fleet_env(kw, form), want["actions"]), want)


# ---- 3. the paths that were there -------------------------------------------------------------------------------------------------------
FORM_NAMES = ("plain", "info", "final")


def _old_and_new(old, new, actions, ends, **call):
    """The tape through the three entries that were there, in turn (the steps that truncate an episode take the final form), and through
    the new one with ped_model "walk", handed the same outputs step by step (arena_harness.play_ops): state, observation, reward, done,
    info and final_obs are equal bit for bit after every step.  -> the old entries' tape."""
    forms = [FORM_NAMES[2 if end else t % 3] for t, end in enumerate(ends)]
    a = play_ops([old[f] for f in forms], actions, form=forms, **call)
    b = play_ops(new, actions, form=forms, **call, ped_model=0 if "nav" in new else "walk")      # both spellings of the model
    assert_tape_equals(b, a)
    assert not is_fill(a["final"][0])
    return a


def test_walk_through_the_new_nav_entry_is_the_old_entries():
    """ped_model = 0 through ddrl_op_nav_env_step_model against the three entries that were there, on the coverage tape (tests/
    test_ped_avoid_cpu.py anchors it to nav_env_ref's): state, observation, reward, done, info and final_obs, bit for bit, every step."""
    _, _, actions, _, trace, info, _, _ = P.nav_coverage_run("walk", ranges=False)
    ends = (info & 16).any(axis=1)                                      # the steps that truncate an episode take the final form
    assert ends.any()
    old = dict(plain="nav_env_step", info="nav_env_step_info", final="nav_env_step_final")
    a = _old_and_new(old, "nav_env_step_model", actions, ends, seed=R.COVERAGE["seed"], max_steps=R.COVERAGE["max_steps"])
    assert np.array_equal(a["state"][-1], trace[-1][0])                 # and it is the rule book's tape


def test_walk_through_the_new_fleet_entry_is_the_old_entries():
    _, _, actions, _, trace = P.fleet_coverage_run("walk", ranges=False)
    ends = np.stack([(s[4] & 16) != 0 for s in trace]).any(axis=1)
    assert ends.any()
    old = dict(plain="fleet_env_step", info="fleet_env_step", final="fleet_env_step_final")
    a = _old_and_new(old, "fleet_env_step_model", actions, ends, n_robots=F.COVERAGE["n_robots"], seed=F.COVERAGE["seed"],
                     max_steps=F.COVERAGE["max_steps"])
    assert np.array_equal(a["state"][-1], trace[-1][0])


def test_the_envs_without_the_argument_are_the_walk_envs():
    from ddrl4nav_amd.env import DeviceNavEnv, FleetNavEnv
    kw, want = nav_reference(TAPE)
    acts = want["actions"][:40]
    a = play_env(DeviceNavEnv(device="cuda", emit_final_obs=True, **kw), acts)
    assert_tape_equals(play_env(nav_env(kw, "final", ped_model="walk"), acts), a)
    # and "avoid" is another trajectory: on this tape the first pedestrian gives way in step 11
    assert np.array_equal(a["state"][:11], want["state"][:11]) and not np.array_equal(a["state"][11], want["state"][11])
    kw, want = fleet_reference((3, 2, 10, 5, 11, 30, 150, 7))
    a = play_env(FleetNavEnv(device="cuda", emit_info=True, **kw), want["actions"][:60])
    assert_tape_equals(play_env(fleet_env(kw, "info", ped_model="walk"), want["actions"][:60]), a)


# ---- 4. repeats and checkpoints ---------------------------------------------------------------------------------------------------------
def test_repeats_are_bit_identical():
    kw, want = nav_reference(SWEEP[-1])
    assert_tape_equals(play_env(nav_env(kw, "final"), want["actions"]), play_env(nav_env(kw, "final"), want["actions"]))
    kw, want = fleet_reference((3, 4, 10, 5, 11, 30, 150, 7))
    acts = want["actions"][:60]
    assert_tape_equals(play_env(fleet_env(kw, "final"), acts), play_env(fleet_env(kw, "final"), acts))


def test_state_dict_resumes_bit_identically_and_keeps_its_model():
    kw, want = nav_reference(SWEEP[-1])
    env = nav_env(kw, "final")
    play_env(env, want["actions"][:20])
    sd = env.state_dict()
    assert sd["ped_model"] == "avoid" and not sd["state"].is_cuda
    assert_tape_equals(play_env(nav_env(kw, "final"), want["actions"][20:], start=sd), tape_from(want, 20))
    with pytest.raises(ValueError, match="ped_model"):
        nav_env(kw, "final", ped_model="walk").load_state_dict(sd)
    kw, want = fleet_reference((3, 2, 10, 5, 11, 30, 150, 7))
    env = fleet_env(kw, "info")
    play_env(env, want["actions"][:20])
    sd = env.state_dict()
    assert_tape_equals(play_env(fleet_env(kw, "info"), want["actions"][20:60], start=sd), tape_from(want, 20), steps=40)
    with pytest.raises(ValueError, match="ped_model"):
        fleet_env(kw, "info", ped_model="walk").load_state_dict(sd)


# ---- 5. the closed loop -----------------------------------------------------------------------------------------------------------------
LN, LT = 4, 8
LOOP_ENV = dict(seed=31, n_obstacles=10, n_peds=5, max_steps=5)


def test_closed_loop_equals_the_host_driven_rollout():
    """arena_harness.closed_loop, one rollout of an avoid env with NavStatus tracking against a rollout fed by the rule book through
    put_states: the pool rows, the actions, rewards, dones and values, the info words and the status sums."""
    out = closed_loop(nav_env(dict(n_envs=LN, **LOOP_ENV), "info"), P.NavEnvPedRef(LN, ped_model="avoid", **LOOP_ENV), LT, rollouts=1,
                      track_nav_status=True)
    assert out.status.per_env()["episode_num"].sum() >= LN

