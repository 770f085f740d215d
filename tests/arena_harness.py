"""What the arena's GPU tests share (tests/test_nav_env_gpu.py, test_fleet_env_gpu.py, test_nav_status_gpu.py, test_truncation_gpu.py,
test_ped_avoid_gpu.py): the constants and one-liners, the rule books' tapes (record), the same tape on the device through an env
(play_env) or through the ops wrappers (play_ops), the step-by-step comparison of two tapes (assert_tape_equals), the net recipe and
the closed loop of collect_states() against a host-driven rollout (closed_loop).  A tape is one dict of per-step arrays: state, laser,
vector, image, reward, done, info (where there is one), actions (record only), first (the reset's observation, or None) and final, the
terminal observations.  Importing this module touches no device, so the host-side files take `bits` from here too.  A new arena
feature extends this module; its test file keeps its own cases and what only it asserts."""
import types

import numpy as np
import torch

import fleet_env_ref as F
import nav_env_ref as R
import nav_status_ref as S
import ped_avoid_ref as P
import truncation_ref as TR

FILL = 0x5A5A5A5A                                                       # what a buffer holds where no kernel has written
SHAPES = [(1, 960), (5,), (3, 48, 48)]
OBS = ("laser", "vector", "image")
HOSTILE = np.array([[np.nan, np.nan], [np.inf, np.inf], [-np.inf, -np.inf], [1e30, 1e30], [-5.0, -5.0], [np.inf, np.nan], [1e30, -1e30]],
                   np.float32)
POOLS = ("_actions", "_logps", "values", "_dones", "_rewards", "adv", "ret")
LOSS_KEYS = ("PpoTotalLoss", "ActorLoss", "VLoss", "EntLoss")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    """float32 array -> its words: equality below is bitwise (a negative zero is not a zero); any other array as it is."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def close_to(got, want, rel=1e-12):
    """Within rel of `want` entry by entry (float64 sums of a few hundred terms in another order); nan where `want` is nan."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.all(np.abs(got[~nan] - want[~nan]) <= rel * np.abs(want[~nan])))


def filled(*lead):
    """Three fp32 buffers [*lead, ...shape] of the observation's shapes, every word the fill."""
    return [filled_like(*(tuple(lead) + s)) for s in SHAPES]


def filled_like(*shape):
    return torch.full(shape, FILL, dtype=torch.int32, device="cuda").view(torch.float32)


def is_fill(a):
    """Every word of a torch tensor or a numpy array (fp32 or int32) is the fill."""
    a = host(a) if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return bool((a.view(np.int32) == FILL).all())


# ---- the rule book's tape ---------------------------------------------------------------------------------------------------------------
def terminal_observation(model):
    """After model.step: [laser, vector, image] of every row in the state its step ended in, or None for a model that keeps none."""
    if isinstance(model, TR.NavEnvFinalRef):
        return model.final
    if isinstance(model, P.NavEnvPedRef):
        return model.final_obs()[0]
    if isinstance(model, F.FleetEnvRef):
        return TR.fleet_final_obs(model)[0]
    return None


def record(model, steps, rng=None, first_state=None, actions=None, hostile=None):
    """Steps a NavEnvRef, FleetEnvRef, NavEnvPedRef, FleetEnvPedRef or NavEnvFinalRef from a reset (or from first_state) -> the tape.
    Without `actions` it plays nav_env_ref.play's: even rows steer to the goal, odd rows draw a0 ~ U(0.3, 1), a1 ~ U(-1, 1) from rng,
    hostile {step: float32 [k, 2]} overrides whole steps.  Besides the tape's keys: trunc bool [steps, rows], final = [(step, rows,
    [laser, vector, image] of those rows)] for the steps that truncated, and events {name: the model's counts of every step, stacked}."""
    n = model.N
    if first_state is None:
        obs = first = model.reset()
    else:
        model.state[:] = first_state
        obs = first = None
    keys = OBS + ("state", "reward", "done", "actions", "trunc") + (("info",) if hasattr(model, "info") else ())
    out, final, events = {k: [] for k in keys}, [], {k: [] for k in model.events}
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
        rows = model.events["trunc"] != 0
        values = tuple(obs) + (model.state.copy(), reward, done, a, rows) + ((model.info.copy(),) if "info" in out else ())
        for k, v in zip(keys, values):
            out[k].append(v)
        for k in events:
            events[k].append(np.array(model.events[k]))
        fin = terminal_observation(model) if rows.any() else None
        if fin is not None:
            final.append((t, rows, [f[rows] for f in fin]))
    out = {k: np.stack(v) for k, v in out.items()}
    out.update(first=first, final=final, events={k: np.stack(v) for k, v in events.items()})
    return out


def tape_from(tape, k):
    """record's tape from step k on, for an env that resumes there: no first observation."""
    out = {key: (v[k:] if isinstance(v, np.ndarray) else v) for key, v in tape.items()}
    out.update(first=None, final=[(t - k, rows, fin) for t, rows, fin in tape["final"] if t >= k])
    return out


# ---- the same tape on the device --------------------------------------------------------------------------------------------------------
def _read_back(steps, state, obs, reward, done, info, final, has_first):
    """One synchronise, one read-back.  obs [steps + 3, rows, ...]: a row that must keep the fill, the reset's row (which keeps the
    fill too when there was no reset), one row per step, and a last row that must keep the fill."""
    torch.cuda.synchronize()
    obs = [host(o) for o in obs]
    assert all(is_fill(o[:1 if has_first else 2]) and is_fill(o[steps + 2:]) for o in obs)   # nothing outside the rows handed over
    out = {k: o[2:steps + 2] for k, o in zip(OBS, obs)}
    out.update(state=host(state), reward=host(reward), done=host(done), first=[o[1] for o in obs] if has_first else None)
    if info is not None:
        out["info"] = host(info)
    if final is not None:
        out["final"] = [host(f) for f in final]
    return out


def play_env(env, actions, start=None):
    """The tape of a fresh DeviceNavEnv or FleetNavEnv (plain, emit_info or emit_final_obs, either pedestrian model) under actions
    [steps, rows, 2]: every step rendered into its own row of three larger buffers (obs_out) with a row on either side that must keep
    the fill, the terminal observations into filled buffers of their own (final_out), so that a row no step wrote is recognisable; one
    read-back at the end.  start: state words or a state_dict to go on from, not a reset; the reset's row then keeps the fill."""
    steps, n = actions.shape[:2]
    assert env.N == n
    bufs = filled(steps + 3, n)
    final = filled(steps, n) if env.emit_final_obs else None
    state = torch.empty((steps,) + tuple(env.state.shape), dtype=torch.int32, device="cuda")
    reward = torch.empty((steps, n), dtype=torch.float32, device="cuda")
    done = torch.empty((steps, n), dtype=torch.uint8, device="cuda")
    info = torch.empty((steps, n), dtype=torch.int32, device="cuda") if env.emit_info else None
    acts = dev(actions)
    if start is None:
        env.state.fill_(-12345)                                         # reset reads nothing of what was there
        out = env.reset(obs_out=[b[1] for b in bufs])
        assert all(o.data_ptr() == b[1].data_ptr() for o, b in zip(out, bufs))
    elif isinstance(start, np.ndarray):
        env.state.copy_(dev(start))
    else:
        env.load_state_dict(start)
    for t in range(steps):
        o, r, d = env.step(acts[t], obs_out=[b[t + 2] for b in bufs], final_out=None if final is None else [f[t] for f in final])
        assert all(x.data_ptr() == b[t + 2].data_ptr() for x, b in zip(o, bufs)) and r is env.reward and d is env.done
        state[t].copy_(env.state)
        reward[t].copy_(r)
        done[t].copy_(d)
        if info is not None:
            info[t].copy_(env.info)
    return _read_back(steps, state, bufs, reward, done, info, final, start is None)


NO, OPTIONAL, REQUIRED = range(3)
# the seven step wrappers of ddrl4nav_amd.ops: (fleet, takes info, takes final_obs)
STEP_OPS = {"nav_env_step": (False, NO, NO), "nav_env_step_info": (False, REQUIRED, NO), "nav_env_step_final": (False, REQUIRED, REQUIRED),
            "nav_env_step_model": (False, OPTIONAL, OPTIONAL), "fleet_env_step": (True, OPTIONAL, NO),
            "fleet_env_step_final": (True, REQUIRED, REQUIRED), "fleet_env_step_model": (True, OPTIONAL, OPTIONAL)}
FORMS = {"plain": (False, False), "info": (True, False), "final": (True, True)}


def play_ops(entry, actions, form=None, n_robots=None, start=None, max_steps=500, ped_model=None, **arena):
    """play_env's tape through the ops wrappers themselves.  entry: a name of STEP_OPS, or one per step; form: which of its outputs the
    entry is handed ("plain": neither, "info", "final": both), or one per step -- by default all it takes.  arena: seed, n_obstacles,
    n_peds and env0 / world0, for the reset too; start: state words to go on from, not a reset.  info rows that no step was handed
    keep their zeros, final rows their fill."""
    from ddrl4nav_amd import ops
    steps, n = actions.shape[:2]
    entries = [entry] * steps if isinstance(entry, str) else list(entry)
    forms = [form] * steps if form is None or isinstance(form, str) else list(form)
    fleet = STEP_OPS[entries[0]][0]
    lead = (n_robots,) if fleet else ()
    state = torch.full((n // n_robots, 96) if fleet else (n, 64), -12345, dtype=torch.int32, device="cuda")
    states = torch.empty((steps,) + tuple(state.shape), dtype=torch.int32, device="cuda")
    obs, final = filled(steps + 3, n), filled(steps, n)
    reward = torch.zeros((steps, n), dtype=torch.float32, device="cuda")
    done = torch.zeros((steps, n), dtype=torch.uint8, device="cuda")
    info = torch.zeros((steps, n), dtype=torch.int32, device="cuda")
    acts = dev(actions)
    if start is None:
        (ops.fleet_env_reset if fleet else ops.nav_env_reset)(state, *lead, [o[1] for o in obs], **arena)
    else:
        state.copy_(dev(start))
    for t, (name, f) in enumerate(zip(entries, forms)):
        _, takes_info, takes_final = STEP_OPS[name]
        with_info, with_final = (takes_info != NO, takes_final != NO) if f is None else FORMS[f]
        assert STEP_OPS[name][0] == fleet and (with_info or takes_info != REQUIRED) and (with_final or takes_final != REQUIRED)
        assert (takes_info != NO or not with_info) and (takes_final != NO or not with_final)
        outs = ([info[t]] if with_info else []) + ([[x[t] for x in final]] if with_final else [])
        kw = dict(arena, max_steps=max_steps, **({} if ped_model is None else dict(ped_model=ped_model)))
        getattr(ops, name)(state, *lead, acts[t], [o[t + 2] for o in obs], reward[t], done[t], *outs, **kw)
        states[t].copy_(state)
    return _read_back(steps, states, obs, reward, done, info, final, start is None)


# ---- two tapes against each other -------------------------------------------------------------------------------------------------------
def assert_tape_equals(got, want, steps=None):
    """Every step of `got` (a device tape) equals `want` (record's, or another device tape) bit for bit: state words, reward, done, the
    info words where both have them, laser, vector and image; the first observation where both have one; the terminal observations
    where both have them -- against record's, the truncated rows equal the model's and every other row still holds the fill."""
    steps = len(want["state"]) if steps is None else steps
    if got.get("first") is not None and want.get("first") is not None:
        assert all(same(g, w) for g, w in zip(got["first"], want["first"]))
    for t in range(steps):                                              # the first step that differs, if any, names itself
        assert np.array_equal(got["state"][t], want["state"][t]), (t, np.nonzero(got["state"][t] != want["state"][t]))
        assert same(got["reward"][t], want["reward"][t]) and np.array_equal(got["done"][t], want["done"][t]), t
        if "info" in got and "info" in want:
            assert np.array_equal(got["info"][t], want["info"][t]), (t, np.nonzero(got["info"][t] != want["info"][t]))
        for k in OBS:
            assert same(got[k][t], want[k][t]), (t, k, np.nonzero(bits(got[k][t]) != bits(want[k][t])))
    if got.get("final") is None or want.get("final") is None:
        return
    if want["final"] and isinstance(want["final"][0], np.ndarray):      # another device tape: fill and all
        assert all(same(g[:steps], w[:steps]) for g, w in zip(got["final"], want["final"]))
        return
    told = {t: (rows, fin) for t, rows, fin in want["final"]}
    for t in range(steps):
        rows, fin = told.get(t, (np.zeros(got["reward"].shape[1], bool), None))
        for k in range(3):
            assert is_fill(got["final"][k][t][~rows]), (t, OBS[k])       # rows that did not truncate are not written at all
            if fin is not None:
                assert same(got["final"][k][t][rows], fin[k]), (t, OBS[k], np.nonzero(bits(got["final"][k][t][rows]) != bits(fin[k])))


# ---- the net and the closed loop --------------------------------------------------------------------------------------------------------
def make_net(max_batch, seed=13):
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
    net = create_net({"config": cfg, "config_nn": cfg_nn, "config_env": env}, max_batch=max_batch)
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


def assert_status_equals(status, want):
    """Every per-row tensor of a NavStatus equals NavStatusRef's, bit for bit."""
    for name, w in want.per_env().items():
        assert same(host(getattr(status, name)), w), name


def closed_loop(env, model, horizon, rollouts=2, **options):
    """Variant A: a StateRollout driven by collect_states(), the observation rendered in the pool (with track_nav_status among the
    options, the navigation status tracked).  Variant B: an identically seeded net whose StateRollout is fed by the host model through
    put_states, stepped with the actions read back.  `rollouts` rollouts with learn() and carry_over() after each: the pools, the
    bootstrap row, the pool rows, the env's state, the losses, every parameter, ro.returns and the status equal the model's.
    -> namespace(ra, rb, rewards, dones, infos, status: NavStatusRef or None)."""
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.nn import GenericPPO
    from ddrl4nav_amd.runner.device_loop import collect_states
    n, T = env.N, horizon
    net_a, net_b = make_net(n * T), make_net(n * T)
    assert isinstance(net_a, GenericPPO) and net_a.continuous
    tracked = bool(options.get("track_nav_status"))
    ra = StateRollout(net_a, n, SHAPES, horizon=T, track_returns=True, **options)
    rb = StateRollout(net_b, n, SHAPES, horizon=T, track_returns=True, **{k: v for k, v in options.items() if k != "track_nav_status"})
    assert [tuple(r.shape) for r in ra.state_rows(3)] == [(n,) + s for s in SHAPES]
    assert all(r.data_ptr() == p[3].data_ptr() for r, p in zip(ra.state_rows(3), ra.states))
    before = net_a.params.clone()
    all_r, all_d, all_w = [], [], []
    for r in range(rollouts):
        collect_states(ra, env)
        if r == 0:
            rb.put_states(0, [dev(x) for x in model.reset()])
        for t in range(T):
            obs, reward, done = model.step(host(rb.act(t)))
            rb.record(t, reward, done)
            rb.put_states(t + 1, [dev(x) for x in obs])
            all_r.append(reward)
            all_d.append(done)
            if tracked:
                all_w.append(model.info.copy())
        rb.bootstrap()
        rb.finish()
        assert ra.rollouts == rb.rollouts == r + 1
        sa, sb = snapshot(ra), snapshot(rb)
        for k in POOLS:
            assert torch.equal(sa[k][:T], sb[k][:T]), (r, k)
        assert torch.equal(sa["values"], sb["values"])                   # the bootstrap row too
        assert np.array_equal(host(ra.dones), np.stack(all_d[-T:])) and same(host(ra.rewards), np.stack(all_r[-T:]))
        assert np.array_equal(host(env.state), model.state)
        assert not tracked or np.array_equal(host(ra._infos)[:T], np.stack(all_w[-T:]))
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
    # ro.returns against the model's episode returns (Status.update_reward_status over the steps played)
    rew, don = np.stack(all_r), np.stack(all_d)
    rsum, rep, fin = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    for t in range(rollouts * T):
        rsum += rew[t]
        rep = np.where(don[t] != 0, rsum, rep)
        rsum = np.where(don[t] != 0, np.float32(0), rsum)
        fin += don[t] != 0
    for ro in (ra, rb):
        assert same(host(ro.returns.rewards_episode), rep) and np.array_equal(host(ro.returns.episodes_finished), fin)
        assert same(host(ro.returns.rewards_sum), rsum)
    assert ra.returns.mean_return() == float(rep[fin > 0].astype(np.float32).mean())
    status = None
    if tracked:
        status = S.NavStatusRef(n)
        status.update(np.stack(all_w))
        assert_status_equals(ra.nav_status, status)
    return types.SimpleNamespace(ra=ra, rb=rb, rewards=rew, dones=don, infos=all_w, status=status)
