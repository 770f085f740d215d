"""The pedestrian model "avoid" on the GPU (csrc/navcore.h nav_walk_peds_avoid in the step kernels of csrc/navenv.hip and
csrc/fleetenv.hip) against the integer rule book tests/ped_avoid_ref.py: every state word, lidar range, vector
entry, map cell, reward, done, info word and terminal observation after every step, bit for bit, through every form of both envs; the
"walk" model through the new entry points against the old ones; repeats, checkpoints and the closed loop.  Run with `-m gpu`."""
import functools
import types

import numpy as np
import pytest
import torch

import fleet_env_ref as F
import nav_env_ref as R
import nav_status_ref as S
import ped_avoid_ref as P

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
SHAPES = [(1, 960), (5,), (3, 48, 48)]
FORMS = {"plain": {}, "info": dict(emit_info=True), "final": dict(emit_final_obs=True)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def guarded(n):
    return [torch.full((n,) + s, GUARD, dtype=torch.int32, device="cuda").view(torch.float32) for s in SHAPES]


def is_guard(a):
    return bool((np.ascontiguousarray(a).view(np.int32) == GUARD).all())


# ---- the rule book's tapes: computed once, never modified -------------------------------------------------------------------------------
def record(model, steps, rng, first_state=None, actions=None, hostile=None):
    """Steps a NavEnvPedRef or FleetEnvPedRef from a reset (or from first_state) -> dict of stacked per-step arrays: state, laser, vector,
    image, reward, done, info, and final = [(step, rows, [laser, vector, image] of those rows)] for the steps that truncated."""
    n = model.N
    if first_state is None:
        obs = first = model.reset()
    else:
        model.state[:] = first_state
        obs = first = None
    out = {k: [] for k in ("state", "laser", "vector", "image", "reward", "done", "info", "actions")}
    final = []
    for t in range(steps):
        if actions is not None:
            a = actions[t]
        else:
            a = np.stack([rng.uniform(0.3, 1.0, n), rng.uniform(-1.0, 1.0, n)], axis=1).astype(np.float32)
            if obs is not None:
                a[0::2] = R.steering_actions(obs[1])[0::2]
            if hostile is not None and t in hostile:
                a = np.resize(hostile[t], (n, 2)).astype(np.float32)
        obs, reward, done = model.step(a)
        for k, v in zip(("laser", "vector", "image"), obs):
            out[k].append(v)
        for k, v in (("state", model.state.copy()), ("reward", reward), ("done", done), ("info", model.info.copy()), ("actions", a)):
            out[k].append(v)
        rows = model.events["trunc"] != 0
        if rows.any():
            if isinstance(model, P.NavEnvPedRef):
                fin = model.final_obs()[0]
            else:
                import truncation_ref as TR
                fin = TR.fleet_final_obs(model)[0]
            final.append((t, rows, [f[rows] for f in fin]))
    out = {k: np.stack(v) for k, v in out.items()}
    out["first"], out["final"] = first, final
    return out


HOSTILE = np.array([[np.nan, np.nan], [np.inf, np.inf], [-np.inf, -np.inf], [1e30, 1e30], [-5.0, -5.0], [np.inf, np.nan], [1e30, -1e30]],
                   np.float32)


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


def play(env, actions, reset=True):
    """The trajectory of `env` under actions [steps, rows, 2], the terminal observations rendered into guard-filled buffers of their
    own every step; one read-back at the end.  -> dict like record()'s, final = per step [laser, vector, image] (guards where nothing
    was rendered), first = the reset's observation."""
    steps, n = actions.shape[:2]
    first = [host(o).copy() for o in env.reset()] if reset else None
    keep = {k: [] for k in ("state", "laser", "vector", "image", "reward", "done", "info", "final")}
    acts = dev(actions)
    for t in range(steps):
        fin = guarded(n) if env.emit_final_obs else None
        obs, reward, done = env.step(acts[t], final_out=fin)
        for k, v in zip(("laser", "vector", "image"), obs):
            keep[k].append(v.clone())
        keep["state"].append(env.state.clone())
        keep["reward"].append(reward.clone())
        keep["done"].append(done.clone())
        if env.emit_info:
            keep["info"].append(env.info.clone())
        if fin is not None:
            keep["final"].append(fin)
    torch.cuda.synchronize()
    out = {k: np.stack([host(x) for x in v]) for k, v in keep.items() if v and k != "final"}
    out["final"] = [[host(x) for x in f] for f in keep["final"]]
    out["first"] = first
    return out


def assert_equals_the_model(got, want, steps=None):
    steps = len(want["state"]) if steps is None else steps
    if got["first"] is not None and want["first"] is not None:
        assert all(same(g, w) for g, w in zip(got["first"], want["first"]))
    for t in range(steps):                                              # the first step that differs, if any, names itself
        assert np.array_equal(got["state"][t], want["state"][t]), (t, np.nonzero(got["state"][t] != want["state"][t]))
        assert same(got["reward"][t], want["reward"][t]) and np.array_equal(got["done"][t], want["done"][t]), t
        for k in ("laser", "vector", "image"):
            assert same(got[k][t], want[k][t]), (t, k)
        if "info" in got:
            assert np.array_equal(got["info"][t], want["info"][t]), t
    if got["final"]:
        told = {t: (rows, fin) for t, rows, fin in want["final"] if t < steps}
        for t in range(steps):
            rows = told[t][0] if t in told else np.zeros(got["reward"].shape[1], bool)
            for k in range(3):
                assert is_guard(got["final"][t][k][~rows]), (t, k)            # the rows of the others are not written
                if t in told:
                    assert same(got["final"][t][k][rows], told[t][1][k]), (t, k)


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
    got = {form: play(nav_env(kw, form), want["actions"]) for form in FORMS}
    for form in FORMS:
        assert_equals_the_model(got[form], want)
    assert "info" not in got["plain"] and not got["plain"]["final"] and not got["info"]["final"] and len(got["final"]["final"]) == 300
    for k in ("state", "laser", "vector", "image", "reward", "done"):
        assert np.array_equal(got["plain"][k].view(np.uint8), got["info"][k].view(np.uint8))
        assert np.array_equal(got["plain"][k].view(np.uint8), got["final"][k].view(np.uint8))


SWEEP = [(n, n_obs, n_peds, 1000 + 7 * n_peds, 9, 40, 100 + n) for n in (1, 3) for n_peds in (0, 1, 2, 5) for n_obs in (0, 10)]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "N%d-obs%d-ped%d" % c[:3])
def test_nav_sweep_equals_the_rule_book(case):
    """No other pedestrian, no pedestrian, no obstacle, a non-zero env0, and max_steps = 9: respawn churn."""
    kw, want = nav_reference(case)
    assert want["done"].any() and want["final"]
    assert_equals_the_model(play(nav_env(kw, "final"), want["actions"]), want)


def test_the_branch_states_equal_the_rule_book():
    """The crafted states of tests/test_ped_avoid_cpu.py -- every rank won, the static refusal, everything blocked -- after one step."""
    states = P.branch_states()
    kw = dict(n_envs=len(states), seed=2, max_steps=500, env0=3, **P.BRANCH_POPULATION)
    model = P.NavEnvPedRef(ped_model="avoid", **kw)
    want = record(model, 2, None, first_state=states, actions=np.zeros((2, len(states), 2), np.float32))
    assert all(model.branches[k] > 0 for k in P.BRANCHES)
    env = nav_env(kw, "final")
    env.state.copy_(dev(states))
    assert_equals_the_model(play(env, want["actions"], reset=False), want)


def test_the_head_on_pedestrian_walks_around_the_robot():
    """60 steps of a robot that stands still: the rule book's trajectory, no pedestrian hit; under "walk" the same state is hit."""
    kw = dict(n_envs=1, seed=0, n_obstacles=0, n_peds=1, max_steps=500)
    acts = np.zeros((60, 1, 2), np.float32)
    want = record(P.NavEnvPedRef(ped_model="avoid", **kw), 60, None, first_state=P.head_on_state(), actions=acts)
    env = nav_env(kw, "info")
    env.state.copy_(dev(P.head_on_state()))
    got = play(env, acts, reset=False)
    assert_equals_the_model(got, want)
    assert not ((got["info"] >> 2) & 3).any() and not got["done"].any()
    env = nav_env(kw, "info", ped_model="walk")
    env.state.copy_(dev(P.head_on_state()))
    assert (((play(env, acts, reset=False)["info"] >> 2) & 3) == 2).sum() >= 1


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
    want = record(P.NavEnvPedRef(ped_model="avoid", **kw), 2, None, first_state=words, actions=acts)
    env = nav_env(kw, "final")
    env.state.copy_(dev(words))
    assert_equals_the_model(play(env, acts, reset=False), want)
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
        assert_equals_the_model(play(fleet_env(kw, form), want["actions"]), want)


# ---- 3. the paths that were there -------------------------------------------------------------------------------------------------------
def _both_sides(reset, n_states, words, rows):
    """Two identical sets of tensors for one env each, reset alike: a plays the entries that were there, b the new one."""
    sides = []
    for _ in range(2):
        st = torch.zeros((n_states, words), dtype=torch.int32, device="cuda")
        obs = [torch.zeros((rows,) + s, device="cuda") for s in SHAPES]
        reset(st, obs)
        sides.append(dict(st=st, obs=obs, rw=torch.zeros(rows, device="cuda"), dn=torch.zeros(rows, dtype=torch.uint8, device="cuda"),
                          info=torch.zeros(rows, dtype=torch.int32, device="cuda"), fin=guarded(rows)))
    return sides


def _equal_sides(a, b):
    words = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
    flat = lambda s: [s["st"], s["rw"], s["dn"], s["info"]] + s["obs"] + s["fin"]
    return all(torch.equal(words(x), words(y)) for x, y in zip(flat(a), flat(b)))


def test_walk_through_the_new_nav_entry_is_the_old_entries():
    """ped_model = 0 through ddrl_op_nav_env_step_model against the three entries that were there, on the coverage tape (tests/
    test_ped_avoid_cpu.py anchors it to nav_env_ref's): state, observation, reward, done, info and final_obs, bit for bit, every step."""
    from ddrl4nav_amd import ops
    _, _, actions, _, trace, info, _, _ = P.nav_coverage_run("walk", ranges=False)
    ends = (info & 16).any(axis=1)                                      # the steps that truncate an episode take the final form
    assert ends.any()
    kw = dict(seed=R.COVERAGE["seed"], n_obstacles=10, n_peds=5, max_steps=R.COVERAGE["max_steps"])
    n = R.COVERAGE["n_envs"]
    a, b = _both_sides(lambda st, obs: ops.nav_env_reset(st, obs, seed=kw["seed"]), n, 64, n)
    acts = dev(actions)
    for t in range(len(actions)):
        form = 2 if ends[t] else t % 3                                  # the three forms in turn, both sides the same one
        if form == 0:
            ops.nav_env_step(a["st"], acts[t], a["obs"], a["rw"], a["dn"], **kw)
            ops.nav_env_step_model(b["st"], acts[t], b["obs"], b["rw"], b["dn"], ped_model="walk", **kw)
        elif form == 1:
            ops.nav_env_step_info(a["st"], acts[t], a["obs"], a["rw"], a["dn"], a["info"], **kw)
            ops.nav_env_step_model(b["st"], acts[t], b["obs"], b["rw"], b["dn"], b["info"], ped_model=0, **kw)
        else:
            ops.nav_env_step_final(a["st"], acts[t], a["obs"], a["rw"], a["dn"], a["info"], a["fin"], **kw)
            ops.nav_env_step_model(b["st"], acts[t], b["obs"], b["rw"], b["dn"], b["info"], b["fin"], ped_model="walk", **kw)
        assert _equal_sides(a, b), t
    assert np.array_equal(host(a["st"]), trace[-1][0]) and not is_guard(host(a["fin"][0]))       # and it is the rule book's tape


def test_walk_through_the_new_fleet_entry_is_the_old_entries():
    from ddrl4nav_amd import ops
    _, _, actions, _, trace = P.fleet_coverage_run("walk", ranges=False)
    ends = np.stack([(s[4] & 16) != 0 for s in trace]).any(axis=1)
    assert ends.any()
    kw = dict(seed=F.COVERAGE["seed"], n_obstacles=10, n_peds=5, max_steps=F.COVERAGE["max_steps"])
    nw, nr = F.COVERAGE["n_worlds"], F.COVERAGE["n_robots"]
    a, b = _both_sides(lambda st, obs: ops.fleet_env_reset(st, nr, obs, seed=kw["seed"]), nw, 96, nw * nr)
    acts = dev(actions)
    for t in range(len(actions)):
        form = 2 if ends[t] else t % 3
        if form == 0:
            ops.fleet_env_step(a["st"], nr, acts[t], a["obs"], a["rw"], a["dn"], **kw)
            ops.fleet_env_step_model(b["st"], nr, acts[t], b["obs"], b["rw"], b["dn"], ped_model="walk", **kw)
        elif form == 1:
            ops.fleet_env_step(a["st"], nr, acts[t], a["obs"], a["rw"], a["dn"], a["info"], **kw)
            ops.fleet_env_step_model(b["st"], nr, acts[t], b["obs"], b["rw"], b["dn"], b["info"], ped_model="walk", **kw)
        else:
            ops.fleet_env_step_final(a["st"], nr, acts[t], a["obs"], a["rw"], a["dn"], a["info"], a["fin"], **kw)
            ops.fleet_env_step_model(b["st"], nr, acts[t], b["obs"], b["rw"], b["dn"], b["info"], b["fin"], ped_model=0, **kw)
        assert _equal_sides(a, b), t
    assert np.array_equal(host(a["st"]), trace[-1][0]) and not is_guard(host(a["fin"][0]))


def test_the_envs_without_the_argument_are_the_walk_envs():
    from ddrl4nav_amd.env import DeviceNavEnv, FleetNavEnv
    kw, want = nav_reference(TAPE)
    acts = want["actions"][:40]
    a = play(DeviceNavEnv(device="cuda", emit_final_obs=True, **kw), acts)
    b = play(nav_env(kw, "final", ped_model="walk"), acts)
    for k in ("state", "laser", "vector", "image", "reward", "done", "info"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    # and "avoid" is another trajectory: on this tape the first pedestrian gives way in step 11
    assert np.array_equal(a["state"][:11], want["state"][:11]) and not np.array_equal(a["state"][11], want["state"][11])
    kw, want = fleet_reference((3, 2, 10, 5, 11, 30, 150, 7))
    a = play(FleetNavEnv(device="cuda", emit_info=True, **kw), want["actions"][:60])
    b = play(fleet_env(kw, "info", ped_model="walk"), want["actions"][:60])
    for k in ("state", "laser", "vector", "image", "reward", "done", "info"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ---- 4. repeats and checkpoints ---------------------------------------------------------------------------------------------------------
def test_repeats_are_bit_identical():
    kw, want = nav_reference(SWEEP[-1])
    a, b = play(nav_env(kw, "final"), want["actions"]), play(nav_env(kw, "final"), want["actions"])
    for k in ("state", "laser", "vector", "image", "reward", "done", "info"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    kw, want = fleet_reference((3, 4, 10, 5, 11, 30, 150, 7))
    a, b = play(fleet_env(kw, "final"), want["actions"][:60]), play(fleet_env(kw, "final"), want["actions"][:60])
    for k in ("state", "laser", "vector", "image", "reward", "done", "info"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_state_dict_resumes_bit_identically_and_keeps_its_model():
    kw, want = nav_reference(SWEEP[-1])
    env = nav_env(kw, "final")
    play(env, want["actions"][:20])
    sd = env.state_dict()
    assert sd["ped_model"] == "avoid" and not sd["state"].is_cuda
    resumed = nav_env(kw, "final")
    resumed.load_state_dict(sd)
    got = play(resumed, want["actions"][20:], reset=False)
    tail = {k: (v[20:] if isinstance(v, np.ndarray) else v) for k, v in want.items()}
    tail["final"] = [(t - 20, rows, fin) for t, rows, fin in want["final"] if t >= 20]
    assert_equals_the_model(got, tail)
    with pytest.raises(ValueError, match="ped_model"):
        nav_env(kw, "final", ped_model="walk").load_state_dict(sd)
    kw, want = fleet_reference((3, 2, 10, 5, 11, 30, 150, 7))
    env = fleet_env(kw, "info")
    play(env, want["actions"][:20])
    sd = env.state_dict()
    resumed = fleet_env(kw, "info")
    resumed.load_state_dict(sd)
    got = play(resumed, want["actions"][20:60], reset=False)
    assert np.array_equal(got["state"], want["state"][20:60]) and np.array_equal(got["info"], want["info"][20:60])
    with pytest.raises(ValueError, match="ped_model"):
        fleet_env(kw, "info", ped_model="walk").load_state_dict(sd)


# ---- 5. the closed loop -----------------------------------------------------------------------------------------------------------------
LN, LT = 4, 8
LOOP_ENV = dict(seed=31, n_obstacles=10, n_peds=5, max_steps=5)


def make_net(seed=13):
    """tests/test_nav_env_gpu.py's net: NavPreNet1D x2 + GaussionActor(2) through create_net, hashed weights."""
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
    net = create_net({"config": cfg, "config_nn": cfg_nn, "config_env": env}, max_batch=LN * LT)
    w = hash_weights([(k, tuple(p.shape)) for k, p in net.named_parameters()], seed)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    return net


def test_closed_loop_equals_the_host_driven_rollout():
    """One collect_states rollout of an avoid env with NavStatus tracking against a rollout fed by the rule book through put_states: the
    pool rows, the actions, rewards, dones and values, the info words and the status sums."""
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.runner.device_loop import collect_states
    net_a, net_b = make_net(), make_net()
    ra = StateRollout(net_a, LN, SHAPES, horizon=LT, track_returns=True, track_nav_status=True)
    rb = StateRollout(net_b, LN, SHAPES, horizon=LT, track_returns=True)
    env = nav_env(dict(n_envs=LN, **LOOP_ENV), "info")
    model = P.NavEnvPedRef(LN, ped_model="avoid", **LOOP_ENV)
    collect_states(ra, env)
    rb.put_states(0, [dev(x) for x in model.reset()])
    infos = []
    for t in range(LT):
        obs, reward, done = model.step(host(rb.act(t)))
        rb.record(t, reward, done)
        rb.put_states(t + 1, [dev(x) for x in obs])
        infos.append(model.info.copy())
    rb.bootstrap()
    rb.finish()
    torch.cuda.synchronize()
    for k in ("_actions", "_logps", "values", "_dones", "_rewards", "adv", "ret"):
        assert torch.equal(getattr(ra, k)[:LT], getattr(rb, k)[:LT]), k
    for pa, pb in zip(ra.states, rb.states):
        assert torch.equal(pa.view(torch.int32), pb.view(torch.int32))
    assert np.array_equal(host(env.state), model.state) and np.array_equal(host(ra._infos)[:LT], np.stack(infos))
    want = S.NavStatusRef(LN)
    want.update(np.stack(infos))
    per_env = want.per_env()
    for name, t in ra.nav_status.named_tensors().items():
        assert same(host(t), per_env[name]), name
    assert per_env["episode_num"].sum() >= LN
