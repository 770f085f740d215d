"""Partial-episode bootstrapping on the GPU against the rule book of tests/truncation_ref.py: the terminal
observation the two env kernels render for a truncated row (csrc/navenv.hip, csrc/fleetenv.hip), the filing of those rows into per-env
pools (csrc/truncate.hip), GAE with the select (csrc/optim.hip) and the closed loop -- DeviceNavEnv / FleetNavEnv(emit_final_obs=True) ->
StateRollout(bootstrap_truncated=S) through collect_states().  Everything is compared bit for bit; every tape asserts its own event
counts.  Run with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

import fleet_env_ref as F
import nav_env_ref as R
import truncation_ref as TR
from arena_harness import FILL, SHAPES, assert_tape_equals, dev, filled, filled_like, host, is_fill, make_net, play_ops, record, same
from oracle import ddrl_oracle as O

pytestmark = pytest.mark.gpu

TRUNC = TR.TRUNC_BIT


def check_tape(final_entry, plain_entry, want, **call):
    """The rule book's tape through the entry that renders the terminal observations and through the one that does not
    (arena_harness.play_ops): state, observation, reward, done and info are bit-identical between the two and the model's, the truncation
    bit is set in the model's rows, those rows of final_obs are the model's and no other row is written at all.  -> the tape."""
    got, plain = play_ops(final_entry, want["actions"], **call), play_ops(plain_entry, want["actions"], **call)
    assert_tape_equals(got, dict(plain, final=None))
    assert all(is_fill(f) for f in plain["final"])
    assert np.array_equal((got["info"] & TRUNC) != 0, want["trunc"])
    assert_tape_equals(got, want)
    return got


# ---- 1. the navigation env ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nav_reference(name):
    """(model kwargs, the tape of NavEnvFinalRef with its terminal observations, event counts) of a tape; never modified."""
    coverage = name == "coverage"
    kw = dict(R.COVERAGE) if coverage else dict(n_envs=5, seed=3, max_steps=3)
    if coverage:                                                        # nav_env_ref.coverage_run, on the model that keeps the snapshots
        want = record(TR.NavEnvFinalRef(**kw), R.COVERAGE_STEPS, np.random.RandomState(0))
    else:
        want = record(TR.NavEnvFinalRef(**kw), 12, actions=np.zeros((12, 5, 2), np.float32))
    ev = want["events"]
    counts = dict(trunc=int(ev["trunc"].sum()), goal=int(ev["goal"].sum()), done=int(want["done"].sum()),
                  collision=int(((ev["wall_hit"] + ev["obstacle_hit"] + ev["ped_hit"]) > 0).sum()))
    return kw, want, counts


def check_nav_tape(name):
    kw, want, counts = nav_reference(name)
    call = dict(env0=kw.get("env0", 0), seed=kw["seed"], n_obstacles=kw.get("n_obstacles", 10), n_peds=kw.get("n_peds", 5))
    got = check_tape("nav_env_step_final", "nav_env_step_info", want, max_steps=kw["max_steps"], **call)
    assert int(got["done"].sum()) == counts["done"]
    return counts, got, want["trunc"]


def test_nav_coverage_tape_renders_the_terminal_observations():
    """N = 8, 300 steps of nav_env_ref's coverage tape: 4 truncations beside 20 collisions and 10 goals."""
    counts, got, trunc = check_nav_tape("coverage")
    assert counts == dict(trunc=4, collision=20, goal=10, done=34), counts
    # a terminal observation is not the next episode's first one: the vector holds the action just played
    assert not same(got["final"][1][trunc], got["vector"][trunc])


def test_nav_truncation_only_tape():
    """N = 5, max_steps = 3, 12 steps of zero actions: every env truncates every third step and nothing else ends an episode."""
    counts, got, trunc = check_nav_tape("truncation_only")
    assert counts == dict(trunc=20, collision=0, goal=0, done=20), counts
    assert trunc[2::3].all() and not trunc[0::3].any() and not trunc[1::3].any()


def test_device_nav_env_owns_its_terminal_observations():
    """DeviceNavEnv(emit_final_obs=True): implies emit_info, owns final_obs, renders elsewhere through final_out; make_device_env reads
    env_final_obs; an env without the option refuses final_out."""
    from ddrl4nav_amd.env import DeviceNavEnv, make_device_env
    _, want, _ = nav_reference("truncation_only")
    actions, told = want["actions"], {t: fin for t, _, fin in want["final"]}
    assert want["trunc"][2].all() and want["trunc"][5].all()            # told[2] and told[5] hold every row
    env = make_device_env({"env_name": "DeviceNav-v0", "env_num": 5, "env_seed": 3, "env_max_steps": 3, "env_final_obs": True})
    assert isinstance(env, DeviceNavEnv) and env.emit_final_obs and env.emit_info and env.info is not None
    assert [tuple(f.shape) for f in env.final_obs] == [(5,) + s for s in SHAPES] and env.truncations_per_rollout(7) == 3
    env.reset()
    elsewhere = filled(5)
    for t in range(6):
        env.step(dev(actions[t]), final_out=elsewhere if t >= 3 else None)
        if t == 2:
            assert all(same(host(f), w) for f, w in zip(env.final_obs, told[2]))
    assert all(same(host(f), w) for f, w in zip(elsewhere, told[5]))
    assert all(same(host(f), w) for f, w in zip(env.final_obs, told[2]))            # untouched since step 2
    plain = DeviceNavEnv(5, device="cuda", seed=3, max_steps=3)
    assert plain.final_obs is None and not plain.emit_info
    with pytest.raises(ValueError, match="emit_final_obs"):
        plain.step(dev(actions[0]), final_out=elsewhere)


# ---- 2. the fleet -------------------------------------------------------------------------------------------------------------------------------------
FLEET_KW = dict(n_worlds=3, seed=5, n_obstacles=10, n_peds=5, max_steps=9)
FLEET_CALL = dict(world0=0, seed=5, n_obstacles=10, n_peds=5, max_steps=9)     # the same, as the ops wrappers take it
FLEET_STEPS = 120


@functools.lru_cache(maxsize=None)
def fleet_reference(nr):
    """(the rule book's tape, world-steps where some but not all robots truncate, truncations); never modified."""
    rng = np.random.RandomState(1)
    actions = np.stack([rng.uniform([0.3, -1.0], [1.0, 1.0], (3 * nr, 2)).astype(np.float32) for _ in range(FLEET_STEPS)])
    want = record(F.FleetEnvRef(n_robots=nr, **FLEET_KW), FLEET_STEPS, actions=actions)
    assert np.array_equal(want["trunc"], (want["info"] & TRUNC) != 0)
    per_world = want["trunc"].reshape(FLEET_STEPS, 3, nr)
    return want, int((per_world.any(axis=2) & ~per_world.all(axis=2)).sum()), int(want["trunc"].sum())


@pytest.mark.parametrize("nr", [1, 2, 4])
def test_fleet_renders_the_terminal_observations(nr):
    """3 worlds x R robots, 120 steps, max_steps = 9: the terminal rows equal observe() of `played` (every robot after all moves, before
    any respawn), also where only some robots of a world truncate; nothing else is written; the other outputs are ddrl_op_fleet_env_step's."""
    want, mixed, total = fleet_reference(nr)
    assert (mixed, total) == {1: (0, 39), 2: (19, 77), 4: (3, 155)}[nr], (mixed, total)
    check_tape("fleet_env_step_final", "fleet_env_step", want, n_robots=nr, **FLEET_CALL)


def test_fleet_truncation_beside_a_collision():
    """A hand-set state, 3 worlds x 2 robots: robot 0 is one step short of max_steps and stands still, robot 1 drives into the wall in
    the same step.  Row 0 of each world is rendered from `played` -- robot 1 still at the wall, not at its respawn -- and row 1 is not
    written."""
    model = F.FleetEnvRef(n_robots=2, **FLEET_KW)
    model.reset()
    model.state[:, F.STEPS] = FLEET_KW["max_steps"] - 1
    model.state[:, 10 + F.X], model.state[:, 10 + F.Y], model.state[:, 10 + F.H] = R.ARENA_R - R.ROBOT_R - 10, 0, 0
    start = model.state.copy()
    model.sanitize()
    assert np.array_equal(model.state, start)
    actions = np.tile(np.array([[0.0, 0.0], [1.0, 0.0]], np.float32), (3, 1))[None]
    want = record(model, 1, first_state=start, actions=actions)
    info = model.info.reshape(3, 2)
    assert (info[:, 0] & TRUNC).all() and not (info[:, 1] & TRUNC).any() and ((info[:, 1] >> 2) & 3 == 1).all() and (info[:, 1] & 64).all()
    assert np.array_equal(want["trunc"][0], np.tile([True, False], 3))
    assert (model.played[:, 10 + F.X] > R.ARENA_R - R.ROBOT_R).all() and (np.abs(model.state[:, 10 + F.X]) <= 2 * R.CELL).all()
    check_tape("fleet_env_step_final", "fleet_env_step", want, n_robots=2, start=start, **FLEET_CALL)


def test_fleet_nav_env_owns_its_terminal_observations():
    from ddrl4nav_amd.env import FleetNavEnv, make_device_env
    want, _, _ = fleet_reference(2)
    actions, trunc, told = want["actions"], want["trunc"], {t: fin for t, _, fin in want["final"]}
    env = make_device_env({"env_name": "DeviceNavFleet-v0", "env_num": 3, "agent_num_per_env": 2, "env_seed": 5, "env_max_steps": 9,
                           "env_final_obs": True})
    assert isinstance(env, FleetNavEnv) and env.emit_final_obs and env.emit_info and env.truncations_per_rollout(20) == 3
    for f in env.final_obs:
        f.view(torch.int32).fill_(FILL)
    env.reset()
    seen = np.zeros(6, bool)
    for t in range(20):
        env.step(dev(actions[t]))
        got = [host(f) for f in env.final_obs]
        seen |= trunc[t]
        assert all(is_fill(g[~seen]) for g in got) and (t not in told or all(same(g[trunc[t]], w) for g, w in zip(got, told[t])))
    assert seen.sum() >= 4
    with pytest.raises(ValueError, match="emit_final_obs"):
        FleetNavEnv(3, 2, device="cuda").step(dev(actions[0]), final_out=env.final_obs)


# ---- 3. filing the rows ---------------------------------------------------------------------------------------------------------------------------------
WIDTHS = (960, 5, 6912)


@pytest.mark.parametrize("flags", ["none", "all", "alternating"])
@pytest.mark.parametrize("n", [1, 7, 65])
def test_file_flagged_rows(n, flags):
    """S = 2, the three row widths of the observation (the vector's 20 bytes move in 4-byte units), counts preset to 0, 1, 2, 3 over the
    envs: a full pool gives slot -1, no write, and a count that still rises."""
    from ddrl4nav_amd import ops
    S = 2
    rng = np.random.RandomState(n)
    flagged = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": np.arange(n) % 2 == 0}[flags]
    info = np.where(flagged, TRUNC | 1, rng.randint(0, 16, n) | (rng.randint(0, 2 ** 10, n) << 5)).astype(np.int32)   # any bit but bit 4
    count = ((np.arange(n) // 2) % 4).astype(np.int32)                  # 0, 0, 1, 1, 2, 2, 3, 3: every count meets both flags
    srcs = [rng.normal(size=(n,) + s).astype(np.float32) for s in SHAPES]
    assert [s[0].size for s in srcs] == list(WIDTHS)
    pools = filled(S, n)
    want_pools, want_count = [host(p).copy() for p in pools], count.copy()
    want_slot = TR.file_rows_ref(info, srcs, want_pools, want_count)
    got_count, got_slot = dev(count), torch.full((n,), 77, dtype=torch.int32, device="cuda")
    out = ops.file_flagged_rows(dev(info), list(zip([dev(s) for s in srcs], pools)), got_count, got_slot)
    assert out is got_slot
    assert np.array_equal(host(got_slot), want_slot) and np.array_equal(host(got_count), want_count)
    assert all(same(host(p), w) for p, w in zip(pools, want_pools))
    filed = int((want_slot >= 0).sum())
    assert filed == int((flagged & (count < S)).sum()) and (flags == "none") == (filed == 0)
    assert np.array_equal(want_count - count, flagged.astype(np.int32))
    if flags == "all" and n >= 7:
        assert (want_count > S).any() and (want_slot[count >= S] == -1).all()
    # a part on bases that are not 16-byte aligned moves in 4-byte units and files the same rows
    flat = torch.zeros(n * 960 + 4, dtype=torch.float32, device="cuda")
    src = flat[1:1 + n * 960].view(n, 1, 960).copy_(dev(srcs[0]))
    pool = filled(S, n)[0]
    ops.file_flagged_rows(dev(info), [(src, pool)], dev(count), got_slot)
    assert src.data_ptr() % 16 == 4 and same(host(pool), want_pools[0]) and np.array_equal(host(got_slot), want_slot)


# ---- 4. GAE with the select -------------------------------------------------------------------------------------------------------------------------------
def gae_case(T, N, S, seed):
    rng = np.random.RandomState(seed)
    values, rewards = rng.normal(size=(T + 1, N)).astype(np.float32), rng.normal(size=(T, N)).astype(np.float32)
    dones = (rng.uniform(size=(T, N)) < 0.3).astype(np.uint8)
    dones[T // 2, N // 2] = 1
    slots = np.where((dones != 0) & (rng.uniform(size=(T, N)) < 0.6), rng.randint(0, S, (T, N)), -1).astype(np.int32)
    slots[T // 2, N // 2] = S - 1
    boot = rng.normal(size=(S, N)).astype(np.float32)
    return values, rewards, dones, slots, boot


def gae_on_device(values, rewards, dones, slots, boot, gamma=0.99, landa=0.95):
    from ddrl4nav_amd import ops
    T, N = rewards.shape
    adv, ret = filled_like(T, N), filled_like(T, N)
    ops.gae_bootstrap(dev(values), dev(rewards), dev(dones), dev(slots), dev(boot), gamma, landa, adv, ret)
    return host(adv), host(ret)


@pytest.mark.parametrize("N", [1, 64, 65])
@pytest.mark.parametrize("T", [1, 5, 33])
def test_gae_bootstrap_equals_the_fp32_model(T, N):
    from ddrl4nav_amd.agent import gae_device
    S = 3
    values, rewards, dones, slots, boot = gae_case(T, N, S, 100 * T + N)
    assert (slots >= 0).any() and (slots < 0).any() or T * N == 1
    want = TR.gae_bootstrap_ref(values, rewards, dones, slots, boot)
    got = gae_on_device(values, rewards, dones, slots, boot)
    assert same(got[0], want[0]) and same(got[1], want[1])
    # a NaN in every boot entry that no slot names changes nothing
    named = np.zeros((S, N), bool)
    named[slots[slots >= 0], np.nonzero(slots >= 0)[1]] = True
    holes = np.where(named, boot, np.float32(np.nan))
    got_holes = gae_on_device(values, rewards, dones, slots, holes)
    assert same(got_holes[0], want[0]) and same(got_holes[1], want[1]) and (np.isnan(holes).any() or named.all())
    # all slots -1: ddrl_gae, bit for bit, whatever boot holds
    none = np.full((T, N), -1, np.int32)
    plain = gae_on_device(values, rewards, dones, none, np.full((S, N), np.nan, np.float32))
    adv, ret = gae_device(dev(values), dev(rewards), dev(dones), 0.99, 0.95)
    oadv, oret = O.gae(values, rewards, dones)
    assert same(plain[0], host(adv)) and same(plain[1], host(ret)) and same(plain[0], oadv) and same(plain[1], oret)
    # slots outside [-1, S) act as -1
    wild = np.where(slots >= 0, slots, np.where(dones != 0, S, -5)).astype(np.int32)
    assert ((wild >= S).any() or not ((dones != 0) & (slots < 0)).any()) and ((wild < -1).any() or (dones != 0).all())
    if slots[0, 0] < 0:
        wild[0, 0] = np.iinfo(np.int32).min if dones[0, 0] == 0 else np.iinfo(np.int32).max
    got_wild = gae_on_device(values, rewards, dones, wild, holes)
    assert same(got_wild[0], want[0]) and same(got_wild[1], want[1])


# ---- 5. the closed loop -------------------------------------------------------------------------------------------------------------------------------------
N_ENVS, T, MAX_STEPS = 6, 7, 3


def make_pair(fleet):
    """(device env with emit_final_obs, host model with the same rules)."""
    from ddrl4nav_amd.env import DeviceNavEnv, FleetNavEnv
    if fleet:
        kw = dict(seed=31, n_obstacles=10, n_peds=5, max_steps=MAX_STEPS)
        return FleetNavEnv(3, 2, device="cuda", emit_final_obs=True, **kw), F.FleetEnvRef(3, 2, **kw)
    kw = dict(seed=31, n_obstacles=10, n_peds=5, max_steps=MAX_STEPS)
    return DeviceNavEnv(N_ENVS, device="cuda", emit_final_obs=True, **kw), TR.NavEnvFinalRef(N_ENVS, **kw)


def model_step(model, actions):
    """One step of either host model -> (reward, done, info words or None, terminal observation, truncated rows)."""
    _, reward, done = model.step(actions)
    if isinstance(model, F.FleetEnvRef):
        final, rows = TR.fleet_final_obs(model)
        return reward, done, model.info.copy(), final, rows
    return reward, done, None, model.final, model.truncated


def run_closed_loop(S, fleet=False, normalize=False):
    """Two chained collect_states() calls; after each, the host model replays the actions the rollout took and files its own terminal
    observations, and everything the feature adds is compared with it.  -> (truncations seen, truncations dropped) per rollout."""
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.runner.device_loop import collect_states
    net = make_net(N_ENVS * T)
    env, model = make_pair(fleet)
    assert env.N == N_ENVS and env.truncations_per_rollout(T) == 3
    ro = StateRollout(net, env.N, SHAPES, horizon=T, bootstrap_truncated=S, normalize_obs=normalize or None, normalize_returns=normalize,
                      track_returns=True)
    assert [tuple(p.shape) for p in ro.final_pools] == [(S, N_ENVS) + s for s in SHAPES] and tuple(ro.slots.shape) == (T + 1, N_ENVS)
    assert tuple(ro.boot.shape) == (S, N_ENVS) and tuple(ro._infos.shape) == (T + 1, N_ENVS) and ro.nav_status is None
    assert set(ro.state_dict()) == {"ret_norm", "obs_norm"}                # unchanged by the option
    model.reset()
    out = []
    for r in range(2):
        affines = [None if n is None else n.affine.clone() for n in ro.obs_norm or [None] * 3]    # frozen until this rollout's finish()
        collect_states(ro, env)
        torch.cuda.synchronize()
        actions = host(ro.actions)
        pools = [np.zeros((S, N_ENVS) + s, np.float32) for s in SHAPES]
        count, slots, seen = np.zeros(N_ENVS, np.int32), np.zeros((T, N_ENVS), np.int32), 0
        for t in range(T):
            reward, done, info, final, rows = model_step(model, actions[t])
            assert same(host(ro.rewards[t]), reward) and np.array_equal(host(ro.dones[t]), done), (r, t)
            got_info = host(ro._infos[t])
            assert np.array_equal((got_info & TRUNC) != 0, rows) and (info is None or np.array_equal(got_info, info))
            slots[t] = TR.file_rows_ref(got_info, final, pools, count)
            seen += int(rows.sum())
        assert np.array_equal(host(env.state), model.state)
        # slots, counts and the filed rows equal the rule book's
        assert np.array_equal(host(ro.slots[:T]), slots) and np.array_equal(host(ro.trunc_count), count)
        dropped = int(np.clip(count - S, 0, None).sum())
        assert ro.truncations_dropped() == dropped and seen == int((slots >= 0).sum()) + dropped
        want_pools = [dev(p) for p in pools]
        if normalize:
            want_pools = [ops.normalize_columns(p.view((S * N_ENVS,) + s), a, 10.0).view(p.shape) for p, a, s in zip(want_pools, affines, SHAPES)]
            assert r == 0 or not same(host(want_pools[0]), pools[0])       # rollout 0: the affine of a fresh state changes nothing
        for got, want in zip(ro.final_pools, want_pools):
            assert same(host(got), host(want))
        # boot is the net's value of the model's pools in the same [S * N] layout
        (_, _), values = net([p.view((S * N_ENVS,) + s) for p, s in zip(want_pools, SHAPES)], play_mode=True)
        boot = host(values[0][:, 0]).reshape(S, N_ENVS)
        assert same(host(ro.boot), boot)
        # adv and ret are the fp32 model's on the rollout's own columns
        rewards = host(ro.rewards_norm if normalize else ro.rewards)
        assert normalize == (not same(rewards, host(ro.rewards)))
        want_adv, want_ret = TR.gae_bootstrap_ref(host(ro.values), rewards, host(ro.dones), slots, boot, ro.gamma, ro.landa)
        assert same(host(ro.adv), want_adv) and same(host(ro.ret), want_ret)
        plain_adv, _ = O.gae(host(ro.values), rewards, host(ro.dones), ro.gamma, ro.landa)
        filed, lost = slots >= 0, (slots < 0) & ((host(ro._infos[:T]) & TRUNC) != 0)
        assert not same(want_adv[filed], plain_adv[filed]) and same(want_adv[lost], plain_adv[lost])   # a dropped step: the terminal treatment
        out.append((seen, dropped))
        ro.carry_over()
        assert int(ro.trunc_count.abs().sum()) == 0
    return out, ro, env


def test_closed_loop_bootstraps_every_truncation():
    """N = 6, T = 7, max_steps = 3, S = truncations_per_rollout(7) = 3: nothing is dropped."""
    out, ro, env = run_closed_loop(3)
    assert all(seen >= N_ENVS and dropped == 0 for seen, dropped in out), out
    assert ro.rollouts == 2 and ro.returns is not None


def test_closed_loop_with_one_slot_drops_the_rest():
    out, _, _ = run_closed_loop(1)
    assert all(dropped > 0 and seen > dropped for seen, dropped in out), out


def test_closed_loop_with_normalised_observations_and_returns():
    out, ro, _ = run_closed_loop(3, normalize=True)
    assert all(dropped == 0 for _, dropped in out) and all(n is not None for n in ro.obs_norm) and ro.ret_norm is not None


def test_closed_loop_on_a_fleet():
    out, _, env = run_closed_loop(3, fleet=True)
    assert env.n_robots == 2 and all(seen >= N_ENVS and dropped == 0 for seen, dropped in out), out


def test_the_loop_refuses_what_is_not_built():
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.env import DeviceNavEnv
    from ddrl4nav_amd.runner.device_loop import collect_states
    net = make_net(N_ENVS * T)
    env = DeviceNavEnv(N_ENVS, device="cuda", max_steps=MAX_STEPS, emit_final_obs=True)
    ro = StateRollout(net, N_ENVS, SHAPES, horizon=T, bootstrap_truncated=2)
    with pytest.raises(ValueError, match="emit_final_obs"):
        collect_states(ro, DeviceNavEnv(N_ENVS, device="cuda", max_steps=MAX_STEPS, emit_info=True))
    with pytest.raises(ValueError, match="keep_step"):
        collect_states(ro, env, keep_step=True)
    with pytest.raises(ValueError, match="keep_step"):
        ro.carry_over(keep_step=True)
    with pytest.raises(ValueError, match="terminal"):
        ro.record(0, env.reward, env.done, info=env.info)
    with pytest.raises(ValueError):
        StateRollout(net, N_ENVS, SHAPES, horizon=T, bootstrap_truncated=-1)
    off = StateRollout(net, N_ENVS, SHAPES, horizon=T)
    assert off.S == 0 and off.final_pools is None and off.slots is None and off._infos is None and off.truncations_dropped() == 0
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        off.record(0, env.reward, env.done, final_obs=env.final_obs)
    collect_states(off, env)                                            # an env that renders them serves a rollout that does not ask
    assert off.rollouts == 1
