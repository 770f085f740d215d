"""Navigation episode statistics on the GPU: the info word of ddrl_op_nav_env_step_info against the rule book
of tests/nav_status_ref.py, the accumulator of csrc/navstat.hip against the reference's own Status (golden F29) and the numpy model, bit
for bit, its reduction against the model's float64, and the closed loop -- DeviceNavEnv(emit_info=True) + StateRollout(
track_nav_status=True) through collect_states.  Run with `-m gpu`."""
import functools
import os

import numpy as np
import pytest
import torch

import nav_status_ref as S
from arena_harness import FILL, HOSTILE, POOLS, SHAPES, close_to, dev, host, is_fill, make_net, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- 1. the info word ------------------------------------------------------------------------------------------------------------------------
STEPS = 300
ENVS, POPULATIONS = (1, 7, 65), ((0, 0), (10, 5), (3, 1))


@functools.lru_cache(maxsize=None)
def info_reference(n, pops):
    """(model kwargs, actions [300][n][2], states / rewards / dones / info words of every step) of one case, from the rule book; never
    modified.  Even envs steer to the goal, odd envs play random actions, three steps are hostile; max_steps = 40 brings truncations.
    The model casts no rays here: the observations are compared between the two kernels, on the device."""
    kw = dict(n_envs=n, seed=50 + n, n_obstacles=pops[0], n_peds=pops[1], max_steps=40, env0=3 * n)
    hostile = {t: np.resize(np.roll(HOSTILE, t, axis=0), (n, 2)) for t in (7, 23, 150)}
    _, actions, _, trace, info, _ = S.play_info(S.NavInfoEnvRef(ranges=False, **kw), STEPS, np.random.RandomState(n + pops[0]), hostile=hostile)
    return kw, actions, np.stack([s[0] for s in trace]), np.stack([s[2] for s in trace]), np.stack([s[3] for s in trace]), info


@pytest.mark.parametrize("pops", POPULATIONS, ids=lambda p: "obs%d-ped%d" % p)
@pytest.mark.parametrize("n", ENVS)
def test_step_info_equals_the_rule_book_and_changes_nothing_else(n, pops):
    """Every info word of 300 steps; state, reward and done equal the model's, and state, observation, reward and done equal, bit for
    bit and after every step, what ddrl_op_nav_env_step gives from the same start."""
    from ddrl4nav_amd.env import DeviceNavEnv
    kw, actions, want_s, want_r, want_d, want_i = info_reference(n, pops)
    told, plain = DeviceNavEnv(device="cuda", emit_info=True, **kw), DeviceNavEnv(device="cuda", **kw)
    assert told.info is not None and plain.info is None
    told.reset()
    plain.reset()
    acts = dev(actions)
    states = torch.empty((STEPS, n, 64), dtype=torch.int32, device="cuda")
    rewards = torch.empty((STEPS, n), dtype=torch.float32, device="cuda")
    dones = torch.empty((STEPS, n), dtype=torch.uint8, device="cuda")
    infos = torch.empty((STEPS, n), dtype=torch.int32, device="cuda")
    differing = torch.zeros((), dtype=torch.int64, device="cuda")
    for t in range(STEPS):
        out = told.step(acts[t])
        assert len(out) == 3 and out[1] is told.reward and out[2] is told.done
        po, pr, pd = plain.step(acts[t])
        states[t].copy_(told.state)
        rewards[t].copy_(told.reward)
        dones[t].copy_(told.done)
        infos[t].copy_(told.info)
        for x, y in zip(out[0] + [told.reward, told.state], po + [pr, plain.state]):
            differing += (x.view(torch.int32) != y.view(torch.int32)).sum()
        differing += (told.done != pd).sum()
    torch.cuda.synchronize()
    assert int(differing.item()) == 0
    got_i = host(infos)
    for t in range(STEPS):                                              # the first step that differs, if any, names itself
        assert np.array_equal(got_i[t], want_i[t]), (t, [hex(w) for w in got_i[t]], [hex(w) for w in want_i[t]])
    assert np.array_equal(host(states), want_s) and same(host(rewards), want_r) and np.array_equal(host(dones), want_d)
    f = S.unpack_info(want_i)
    assert f["done"].any() and (n == 1 or f["truncated"].any()) and (pops[1] > 0) == bool(f["close"].any())


def test_step_info_writes_its_words_and_nothing_around_them():
    from ddrl4nav_amd import ops
    from ddrl4nav_amd._lib import DdrlError
    from ddrl4nav_amd.env import DeviceNavEnv
    kw, actions, _, _, _, want_i = info_reference(7, (10, 5))
    env = DeviceNavEnv(device="cuda", **kw)
    env.reset()
    buf = torch.full((3, 7), FILL, dtype=torch.int32, device="cuda")
    call = dict(env0=env.env0, seed=env.seed, n_obstacles=10, n_peds=5, max_steps=40)
    out = ops.nav_env_step_info(env.state, dev(actions[0]), env.obs, env.reward, env.done, buf[1], **call)
    assert len(out) == 4 and out[3].data_ptr() == buf[1].data_ptr()
    got = host(buf)
    assert np.array_equal(got[1], want_i[0]) and is_fill(got[0]) and is_fill(got[2])
    fields = ops.nav_info_fields(buf[1])
    assert fields["v"].is_cuda and np.array_equal(host(fields["v"]), S.unpack_info(want_i[0])["v"])
    with pytest.raises(AssertionError):
        ops.nav_env_step_info(env.state, dev(actions[0]), env.obs, env.reward, env.done, buf[1].to(torch.int64), **call)
    with pytest.raises(AssertionError):
        ops.nav_env_step_info(env.state, dev(actions[0]), env.obs, env.reward, env.done, buf.view(-1)[:8], **call)
    with pytest.raises(DdrlError):                                       # the info on the reward
        ops.nav_env_step_info(env.state, dev(actions[0]), env.obs, env.reward, env.done, env.reward.view(torch.int32), **call)


# ---- 2. the accumulator ----------------------------------------------------------------------------------------------------------------------
N, T = 24, 400
CHUNKS = (1, 2, 253, 144)                                               # the launches end at the fixture's checkpoints 1, 3, 256, 400


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "f29_nav_status.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def model_of(columns):
    """{checkpoint: per-env arrays} of NavStatusRef over the given columns (a tuple) of the fixture's stream, and the model at the end;
    never modified."""
    words = fixture()["info"][:, list(columns)]
    m, out = S.NavStatusRef(len(columns)), {}
    for t in range(T):
        m.step(words[t])
        if t + 1 in (1, 3, 256, 400):
            out[t + 1] = m.per_env()
    return out, m


COLUMNS = {"all": tuple(range(N)), "one": (17,), "23": tuple(range(1, N)), "tiled300": tuple(k % N for k in range(300))}


def assert_status(st, want, where):
    torch.cuda.synchronize()
    for name, t in st.named_tensors().items():
        assert same(host(t), want[name]), (where, name)


@pytest.mark.parametrize("columns", list(COLUMNS))
@pytest.mark.parametrize("chunks", [(T,), CHUNKS], ids=["one_launch", "four_launches"])
def test_update_equals_the_reference_and_the_model(chunks, columns):
    from ddrl4nav_amd.agent import NavStatus
    cols = COLUMNS[columns]
    g, (want, _) = fixture(), model_of(cols)
    words = dev(g["info"][:, list(cols)])
    st = NavStatus(len(cols), "cuda")
    st.update(words[:0])                                                # T == 0: nothing happens
    assert_status(st, S.NavStatusRef(len(cols)).per_env(), "empty")
    t = 0
    for rows in chunks:
        st.update(words[t:t + rows])
        t += rows
        assert_status(st, want[t], t)
        for name in S.PER_ENV:                                          # and the reference's own arrays, column for column
            if name != "trunc_num":
                assert same(host(getattr(st, name)), np.ascontiguousarray(g["c%d_%s" % (t, name)][..., list(cols)])), (t, name)
    assert t == T and (columns == "one" or int(st.episode_num.max()) > S.WINDOW)


def test_update_refuses_what_it_cannot_take():
    from ddrl4nav_amd import ops
    from ddrl4nav_amd._lib import DdrlError
    from ddrl4nav_amd.agent import NavStatus
    st = NavStatus(N, "cuda")
    words = dev(fixture()["info"])
    with pytest.raises(ValueError):
        st.update(words[:, :5])
    with pytest.raises(ValueError):
        st.update(words.t()[:N, :N])
    with pytest.raises(TypeError):
        st.update(words.to(torch.int64))
    with pytest.raises(DdrlError):                                       # the words inside the rings
        ops.nav_status_update(st.rings.view(torch.int32).view(-1)[:2 * N].view(2, N), st.sums, st.episode_num, st.rings)
    sd = st.state_dict()
    st.update(words)
    other = NavStatus(N, "cuda")
    other.load_state_dict(st.state_dict())
    assert_status(other, model_of(COLUMNS["all"])[0][400], "loaded")
    st.load_state_dict(sd)
    assert_status(st, S.NavStatusRef(N).per_env(), "restored")


# ---- 3. the reduction ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("columns", ["all", "one", "tiled300"])
def test_reduce_and_summary_equal_the_model(columns):
    from ddrl4nav_amd.agent import NavStatus
    cols = COLUMNS[columns]
    _, m = model_of(cols)
    st = NavStatus(len(cols), "cuda")
    st.update(dev(fixture()["info"][:, list(cols)]))
    first = st.partial().clone()
    again = st.partial().clone()
    torch.cuda.synchronize()
    got, want = host(first), m.partial()
    print(got, want)
    assert np.array_equal(got.view(np.int64), host(again).view(np.int64))         # a fixed order: the same bits
    assert np.array_equal(got[1::2], want[1::2]) and close_to(got, want)
    summary, wanted = st.summary(), m.summary()
    assert tuple(summary) == S.SUMMARY_KEYS and all(np.isfinite(v) for v in summary.values())
    assert close_to([summary[k] for k in S.SUMMARY_KEYS], [wanted[k] for k in S.SUMMARY_KEYS])
    assert summary == st.summary(partials=[got])


def test_summary_of_partials_and_of_an_unfinished_status():
    from ddrl4nav_amd.agent import NavStatus
    words = fixture()["info"]
    _, whole = model_of(COLUMNS["all"])
    parts = []
    for lo, hi in ((0, 7), (7, 15), (15, 24)):
        st = NavStatus(hi - lo, "cuda")
        st.update(dev(words[:, lo:hi]))
        parts.append(host(st.partial()).copy())
    wanted = whole.summary()
    summary = NavStatus(1, "cuda").summary(partials=parts)
    assert close_to([summary[k] for k in S.SUMMARY_KEYS], [wanted[k] for k in S.SUMMARY_KEYS])
    # nobody has finished an episode: the speed means have no env to count
    st = NavStatus(5, "cuda")
    st.update(dev(np.where(S.unpack_info(words[:2, :5])["done"] != 0, words[:2, :5] & ~1, words[:2, :5]).astype(np.int32)))
    summary = st.summary()
    assert all(np.isnan(summary[k]) for k in S.SPEED_KEYS) and summary["ReducedStepsEpisodeLogger"] == 0
    assert all(np.isfinite(summary[k]) for k in S.RATE_KEYS) and host(st.partial())[9] == 0
    fresh = NavStatus(3, "cuda").summary()
    assert all(np.isnan(fresh[k]) for k in S.SPEED_KEYS) and all(fresh[k] == 0 for k in S.RATE_KEYS)


# ---- 4. the closed loop ----------------------------------------------------------------------------------------------------------------------
LN, LT = 8, 16
LOOP_ENV = dict(seed=21, n_obstacles=10, n_peds=5, max_steps=12)


@pytest.mark.parametrize("keep_step", [False, True])
def test_the_loop_tracks_the_status_and_changes_nothing_else(keep_step):
    """Two chained rollouts.  ro.nav_status equals NavStatusRef fed the info words of the model env under the actions the rollouts
    stored: rows 0..T-1 of every rollout, every step once (with keep_step the kept step is counted by the rollout it is carried into).
    The pools, the batch and ro.returns equal those of a run with tracking off."""
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.env import DeviceNavEnv
    from ddrl4nav_amd.runner.device_loop import collect_states
    net_a, net_b = make_net(LN * LT), make_net(LN * LT)
    ra = StateRollout(net_a, LN, SHAPES, horizon=LT, track_returns=True, track_nav_status=True)
    rb = StateRollout(net_b, LN, SHAPES, horizon=LT, track_returns=True)
    assert rb.nav_status is None and ra.nav_status.N == LN and tuple(ra._infos.shape) == (LT + 1, LN)
    env_a, env_b = DeviceNavEnv(LN, device="cuda", emit_info=True, **LOOP_ENV), DeviceNavEnv(LN, device="cuda", **LOOP_ENV)
    with pytest.raises(ValueError, match="emit_info"):
        collect_states(ra, env_b)
    model = S.NavInfoEnvRef(LN, **LOOP_ENV)
    model.reset()
    played = []
    for r in range(2):
        collect_states(ra, env_a, keep_step=keep_step)
        collect_states(rb, env_b, keep_step=keep_step)
        torch.cuda.synchronize()
        acts, infos = host(ra._actions), host(ra._infos)
        for t in range(ra.t0, LT + 1 if keep_step else LT):
            model.step(acts[t])
            assert np.array_equal(infos[t], model.info), (r, t)
            played.append(model.info.copy())
        if keep_step and r > 0:
            assert np.array_equal(infos[0], played[LT])                  # the kept step's words came along
        assert np.array_equal(host(env_a.state), model.state)
        want = S.NavStatusRef(LN)
        want.update(np.stack(played[:(r + 1) * LT]))
        assert_status(ra.nav_status, want.per_env(), r)
        for k in POOLS:
            assert torch.equal(getattr(ra, k), getattr(rb, k)), (r, k)
        for pa, pb in zip(ra.states, rb.states):
            assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), r
        ba, bb = ra.batch(), rb.batch()
        assert all(torch.equal(x, y) for x, y in zip(ba.states, bb.states)) and torch.equal(ba.advs, bb.advs) and torch.equal(ba.actions, bb.actions)
        for k in ("rewards_sum", "rewards_episode", "episodes_finished"):
            assert torch.equal(getattr(ra.returns, k), getattr(rb.returns, k)), (r, k)
        ra.carry_over(keep_step=keep_step)
        rb.carry_over(keep_step=keep_step)
    f = S.unpack_info(np.stack(played))
    assert f["done"].sum() >= 2 * LN and f["truncated"].any()
    summary, wanted = ra.nav_status.summary(), want.summary()
    assert close_to([summary[k] for k in S.SUMMARY_KEYS], [wanted[k] for k in S.SUMMARY_KEYS])
    with pytest.raises(ValueError, match="info"):
        ra.record(ra.t0, env_a.reward, env_a.done)
