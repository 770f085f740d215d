"""Navigation episode statistics without a GPU: the numpy model of tests/nav_status_ref.py against the reference's
own Status (golden F29, tests/golden/make_golden_nav_status.py), the rule book of the info word over the coverage tape, and the host
side of the new entry points -- header against binding, argument checks that come before HIP, the guards of the Python surface."""
import functools
import os
import re
import types

import numpy as np
import pytest

import nav_env_ref as R
import nav_status_ref as S
from arena_abi import BASE, INVALID, ROOT, caller, common_refusals, header_declares, refused
from arena_harness import bits

NEW = ("ddrl_op_nav_env_step_info", "ddrl_op_nav_status_update", "ddrl_op_nav_status_reduce")
N, T = 24, 400
GROUP_KEYS = tuple(k for k in S.SUMMARY_KEYS if k != "TruncationRate")   # what the reference's group_logger returns


@functools.lru_cache(maxsize=None)
def fixture():
    """The arrays of golden F29 (never modified)."""
    with np.load(os.path.join(ROOT, "tests", "golden", "f29_nav_status.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def model_checkpoints():
    """{step: per-env arrays of NavStatusRef after that many steps of the fixture's stream}, and the model after the last."""
    g = fixture()
    m, out = S.NavStatusRef(N), {}
    for t in range(T):
        m.step(g["info"][t])
        if t + 1 in g["checkpoints"]:
            out[t + 1] = m.per_env()
    return out, m


# ---- 1. the model against the reference's Status --------------------------------------------------------------------------------------------
def test_the_fixture_covers_what_it_has_to():
    g = fixture()
    words = g["info"]
    assert words.shape == (T, N) and words.dtype == np.int32 and list(g["checkpoints"]) == [1, 3, 256, 400]
    f = S.unpack_info(words)
    done = f["done"] != 0
    assert all(((f["collision"] == k) & done).any() for k in (1, 2)) and not (f["collision"] == 3).any()
    assert (f["goal"] & f["done"]).any() and f["truncated"].any() and f["wall_hit"].any() and f["obstacle_hit"].any()
    assert (f["close"] == 0).any() and (f["close"] == 1).any()
    assert done.sum(0).max() > S.WINDOW                                   # a ring wraps
    assert (done[:3].sum(0) == 0).any() and (done.sum(0) >= 1).all()
    assert 0.28 < done.mean() < 0.39
    assert (~done & ((f["goal"] != 0) | (f["collision"] != 0))).any()      # a running slot that a later step overwrites
    assert np.array_equal(S.pack_info(*(f[k] for k in ("done", "goal", "collision", "truncated", "close", "wall_hit", "obstacle_hit",
                                                       "v", "w"))), words)
    assert all(("g_" + k) in g and np.isfinite(g["g_" + k]) for k in GROUP_KEYS)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "f29_nav_status.npz")) < 256 * 1024


def test_the_model_equals_the_reference_bit_for_bit():
    g = fixture()
    got, _ = model_checkpoints()
    assert sorted(got) == [1, 3, 256, 400]
    for step, arrays in got.items():
        for name in S.PER_ENV:
            if name == "trunc_num":                                     # not the reference's: the same rule as arrive_num, below
                continue
            want = g["c%d_%s" % (step, name)]
            assert want.dtype == arrays[name].dtype and want.shape == arrays[name].shape, (step, name)
            assert np.array_equal(bits(want), bits(arrays[name])), (step, name)
    assert (g["c3_episode_num"] == 0).any() and (g["c400_episode_num"] >= 1).all() and g["c400_episode_num"].max() > S.WINDOW
    assert not g["c400_coll_robot_num"].any()


def test_the_truncation_ring_follows_the_ring_rule():
    """trunc_num is arrive_num's rule on another bit: the model fed the stream with goal and truncation bits exchanged."""
    words = fixture()["info"].astype(np.int64)
    swapped = (words & ~0x12) | ((words >> 3) & 0x02) | ((words << 3) & 0x10)
    _, m = model_checkpoints()
    other = S.NavStatusRef(N)
    other.update(swapped.astype(np.int32))
    assert np.array_equal(other.arrive_num, m.trunc_num) and np.array_equal(other.trunc_num, m.arrive_num) and m.trunc_num.any()


def test_the_summary_equals_group_logger():
    g = fixture()
    _, m = model_checkpoints()
    got = m.summary()
    assert tuple(got) == S.SUMMARY_KEYS
    for k in S.RATE_KEYS[:3]:                                           # float64 quotients, numpy's own sum: 1e-15 relative
        want = float(g["g_" + k])
        print(k, got[k], want)
        assert want > 0 and abs(got[k] - want) <= 1e-15 * abs(want), k
    # The reference takes numpy's float32 mean of the 24 per-env values: 8 accumulators of 3 adds, 7 combining adds, one division, at
    # most 11 roundings of relative size 2^-24 on partial sums below 24 max|x|; the mean therefore moves by at most 11 * 2^-24 * max|x|.
    # 16 leaves a small margin.  The model sums the same float32 quotients in float64.
    quotients = {"ReducedStepsEpisodeLogger": m.steps_episode}
    for family, name in zip(S.FAMILIES, ("", "CloseHuman", "OpenArea")):
        steps = getattr(m, "steps_episode" + family)
        assert (steps > 0).all()
        quotients["Reduced%sLinearVelocityEpisodeLogger" % name] = getattr(m, "v_speeds_episode" + family) / steps
        quotients["Reduced%sAngularVelocityEpisodeLogger" % name] = getattr(m, "w_speeds_episode" + family) / steps
    assert set(quotients) == set(S.SPEED_KEYS) | {"ReducedStepsEpisodeLogger"}
    for k, x in quotients.items():
        want, bound = float(g["g_" + k]), 16 * 2.0 ** -24 * float(np.abs(x).max())
        print(k, got[k], want, bound)
        assert abs(got[k] - want) <= bound, k
    assert 0 <= got["TruncationRate"] <= 1 and got["TruncationRate"] == np.sum(np.sum(m.trunc_num, 0) / np.clip(m.episode_num + 1, 1, 100)) / N


def test_an_unfinished_status_has_no_speed_means():
    m = S.NavStatusRef(3)
    m.update(S.pack_info(0, 0, 0, 0, [0, 1, 0], 0, 0, [3, 4, 5], [-2, 0, 7])[None].repeat(4, axis=0))
    s = m.summary()
    assert all(np.isnan(s[k]) for k in S.SPEED_KEYS) and all(s[k] == 0 for k in S.RATE_KEYS) and s["ReducedStepsEpisodeLogger"] == 0
    assert not m.episode_num.any() and np.array_equal(m.steps_sum, np.float32([4, 4, 4])) and np.array_equal(m.steps_sum_close_human, np.float32([0, 4, 0]))


def test_combine_of_a_three_way_split_equals_the_whole():
    from ddrl4nav_amd.agent import NavStatus
    words = fixture()["info"]
    _, whole = model_checkpoints()
    parts = []
    for lo, hi in ((0, 7), (7, 15), (15, 24)):
        m = S.NavStatusRef(hi - lo)
        m.update(words[:, lo:hi])
        parts.append(m.partial())
    total, want = np.array(NavStatus.combine(parts)), whole.partial()
    assert total.shape == (22,) and np.array_equal(total[1::2], want[1::2]) and total[1] == N
    assert np.all(np.abs(total - want) <= 1e-12 * np.abs(want))
    assert np.array_equal(NavStatus.combine([want.tolist()]), want)
    for bad in ([], [want[:21]]):
        with pytest.raises(ValueError):
            NavStatus.combine(bad)


# ---- 2. the rule book of the info word ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def info_tape():
    return S.play_info(S.NavInfoEnvRef(**R.COVERAGE), R.COVERAGE_STEPS, np.random.RandomState(0))


def test_the_info_words_of_the_coverage_tape():
    counts, actions, first, trace, info, played = info_tape()
    plain = R.coverage_run()
    assert counts == plain[0] and all(counts[k] >= 1 for k in R.EVENT_NAMES)
    assert np.array_equal(actions, plain[1])
    for (s, o, r, d), (ps, po, pr, pd) in zip(trace, plain[3]):            # telling what happened changes nothing that happens
        assert np.array_equal(s, ps) and np.array_equal(r, pr) and np.array_equal(d, pd) and all(np.array_equal(a, b) for a, b in zip(o, po))
    f = S.unpack_info(info)
    dones = np.stack([step[3] for step in trace])
    assert np.array_equal(f["done"], dones)
    assert not (info.astype(np.int64) & ~0x00FF3FFF).any()                # the other bits are zero
    # the fields against the events, recomputed here from the played states
    model = S.NavInfoEnvRef(**R.COVERAGE)
    model.reset()
    totals = {k: 0 for k in ("goal", "trunc", "wall_hit", "obstacle_hit", "ped_kind", "static_and_ped")}
    for t in range(R.COVERAGE_STEPS):
        model.step(actions[t])
        ev = model.events
        v, w = R.decode_actions(actions[t])
        assert np.array_equal(model.info, info[t]) and np.array_equal(model.played, played[t])
        assert np.array_equal(f["goal"][t], ev["goal"]) and np.array_equal(f["truncated"][t], ev["trunc"])
        assert np.array_equal(f["wall_hit"][t], ev["wall_hit"]) and np.array_equal(f["obstacle_hit"][t], ev["obstacle_hit"])
        static = (ev["wall_hit"] | ev["obstacle_hit"]) != 0
        assert np.array_equal(f["collision"][t], np.where(static, 1, np.where(ev["ped_hit"] != 0, 2, 0)))
        assert np.array_equal(f["done"][t], ((f["collision"][t] != 0) | (f["goal"][t] != 0) | (f["truncated"][t] != 0)).astype(np.int64))
        assert np.array_equal(f["v"][t], v) and np.array_equal(f["w"][t], w)
        assert np.array_equal(played[t][:, R.V], v) and np.array_equal(played[t][:, R.W], w)
        p = played[t].astype(np.int64)
        d2 = np.stack([(p[:, R.X] - p[:, R.PED0 + 4 * j]) ** 2 + (p[:, R.Y] - p[:, R.PED0 + 4 * j + 1]) ** 2 for j in range(5)])
        assert np.array_equal(f["close"][t], (d2 <= S.CLOSE ** 2).any(axis=0).astype(np.int64))
        assert ((d2 < (R.ROBOT_R + R.PED_R) ** 2).any(axis=0) == (ev["ped_hit"] != 0)).all()
        for k in ("goal", "trunc", "wall_hit", "obstacle_hit"):
            totals[k] += int(ev[k].sum())
        totals["ped_kind"] += int((f["collision"][t] == 2).sum())
        totals["static_and_ped"] += int((static & (ev["ped_hit"] != 0)).sum())
    print(totals)
    assert all(totals[k] >= 1 for k in ("goal", "trunc", "wall_hit", "obstacle_hit", "ped_kind"))
    assert (f["close"] == 0).any() and (f["close"] == 1).any()
    assert f["v"].max() == 32                                            # full speed is played
    assert f["w"].min() < 0 < f["w"].max()


def test_no_pedestrians_are_never_close():
    model = S.NavInfoEnvRef(5, seed=3, n_obstacles=4, n_peds=0, max_steps=9)
    *_, info, played = S.play_info(model, 30, np.random.RandomState(1))
    f = S.unpack_info(info)
    assert not f["close"].any() and not (f["collision"] == 2).any() and f["truncated"].any()


def test_info_fields_unpack_like_the_rule_book():
    import torch
    from ddrl4nav_amd import ops
    words = fixture()["info"]
    got, want = ops.nav_info_fields(torch.from_numpy(words)), S.unpack_info(words)
    assert tuple(got) == ops.NAV_INFO_FIELDS == tuple(want)
    for k in want:
        assert got[k].dtype == torch.int32 and np.array_equal(got[k].numpy(), want[k]), k
    assert (ops.NAV_COLLISION_STATIC, ops.NAV_COLLISION_PED) == (1, 2)
    with pytest.raises(AssertionError):
        ops.nav_info_fields(torch.zeros(3))


# ---- 3. header, binding, argument checks, guards --------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_binds():
    from ddrl4nav_amd import _lib, ops
    text, _ = header_declares(NEW, [15, 7, 6])
    assert len(_lib.SIGNATURES["ddrl_op_nav_env_step"][1]) == 14          # the plain entry keeps its signature
    for macro, value in (("ROWS", ops.NAV_STATUS_ROWS), ("RINGS", ops.NAV_STATUS_RINGS), ("WINDOW", ops.NAV_STATUS_WINDOW),
                         ("SUMMARY", ops.NAV_STATUS_SUMMARY)):
        assert re.search(r"#define\s+DDRL_NAV_STATUS_%s\s+%d\b" % (macro, value), text), macro
    assert (ops.NAV_STATUS_ROWS, ops.NAV_STATUS_RINGS, ops.NAV_STATUS_WINDOW) == (len(S.FAMILIES) * len(S.ROWS), len(S.RINGS), S.WINDOW)
    assert ops.NAV_STATUS_SUMMARY == 2 * len(S.SUMMARY_KEYS)
    from ddrl4nav_amd.agent.statistics import NAV_SUMMARY_KEYS
    assert NAV_SUMMARY_KEYS == S.SUMMARY_KEYS


def test_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses: every refusal below is decided before the first HIP call."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    OK = 0
    # the info word among the outputs (arena_abi.common_refusals): null, misaligned, on either end of every other argument and they on it
    bad = common_refusals("ddrl_op_nav_env_step_info") + [dict(n=0), dict(n=-1), dict(e0=2 ** 32 - 7)]
    bad += [dict(info=BASE["dn"] - 28), dict(dn=BASE["info"] + 31)]     # its last word on the dones' first bytes, the dones on its last byte
    refused(caller(lib, "ddrl_op_nav_env_step_info"), bad)

    a, M, n = 0x10000000, 0x1000000, 24
    sb = dict(info=a, sums=a + M, ep=a + 2 * M, rings=a + 3 * M, out=a + 4 * M)
    nbytes = dict(info=400 * n * 4, sums=18 * n * 4, ep=n * 4, rings=5 * 100 * n * 4, out=22 * 8)

    def update(info=sb["info"], T=400, N=n, sums=sb["sums"], ep=sb["ep"], rings=sb["rings"]):
        return lib.ddrl_op_nav_status_update(info, T, N, sums, ep, rings, None)

    bad = [dict(info=None), dict(sums=None), dict(ep=None), dict(rings=None), dict(T=-1), dict(N=0), dict(N=-5), dict(info=a + 2),
           dict(sums=a + M + 1), dict(ep=a + 2 * M + 2), dict(rings=a + 3 * M + 3), dict(T=0, sums=None), dict(T=0, N=0)]
    for p, q in ((p, q) for p in ("info", "sums", "ep", "rings") for q in ("sums", "ep", "rings") if p != q):
        bad += [{q: sb[p]}, {q: sb[p] + nbytes[p] - 4}]
    bad += [dict(info=sb["sums"] - 4 * n * 400 + 4), dict(info=sb["rings"] + 5 * 100 * n * 4 - 4)]
    for kw in bad:
        assert update(**kw) == INVALID, kw
    assert update(T=0) == OK and update(T=0, info=None) == OK           # nothing to do: no launch, on any host

    def reduce(sums=sb["sums"], ep=sb["ep"], rings=sb["rings"], N=n, out=sb["out"]):
        return lib.ddrl_op_nav_status_reduce(sums, ep, rings, N, out, None)

    bad = [dict(sums=None), dict(ep=None), dict(rings=None), dict(out=None), dict(N=0), dict(out=sb["out"] + 4), dict(sums=a + M + 2)]
    bad += [dict(out=sb[p]) for p in ("sums", "ep", "rings")] + [dict(out=sb["rings"] + nbytes["rings"] - 8), dict(ep=sb["sums"] + 4)]
    for kw in bad:
        assert reduce(**kw) == INVALID, kw


def test_the_python_surface_and_its_guards():
    import torch
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.agent import NavStatus, StateRollout
    from ddrl4nav_amd.env import DeviceNavEnv, make_device_env
    from ddrl4nav_amd.runner import device_loop
    assert DeviceNavEnv(4, device="cpu").info is None and not DeviceNavEnv(4, device="cpu").emit_info
    env = DeviceNavEnv(4, device="cpu", emit_info=True)
    assert env.emit_info and env.info.dtype == torch.int32 and tuple(env.info.shape) == (4,)
    cfg = {"env_name": "DeviceNav-v0", "env_num": 3}
    assert make_device_env(cfg, device="cpu").info is None and make_device_env(dict(cfg, env_info=True), device="cpu").info is not None
    # a rollout that tracks needs an env that tells
    tracking = types.SimpleNamespace(T=4, N=4, nav_status=object())
    with pytest.raises(ValueError, match="emit_info"):
        device_loop.collect_states(tracking, DeviceNavEnv(4, device="cpu"))
    with pytest.raises(ValueError, match="4 envs"):
        device_loop.collect_states(types.SimpleNamespace(T=4, N=5, nav_status=object()), env)
    # ... and record() its words
    fake = types.SimpleNamespace(t0=0, _infos=torch.zeros((5, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="info"):
        StateRollout.record(fake, 0, torch.zeros(4), torch.zeros(4, dtype=torch.uint8))
    # host tensors are refused by the wrappers, not handed to a kernel
    st = NavStatus(4, "cpu")
    obs = [torch.zeros((4,) + s) for s in ops.NAV_ENV_SHAPES]
    with pytest.raises(AssertionError):
        ops.nav_env_step_info(env.state, torch.zeros((4, 2)), obs, env.reward, env.done, env.info)
    with pytest.raises(AssertionError):
        ops.nav_status_update(torch.zeros((2, 4), dtype=torch.int32), st.sums, st.episode_num, st.rings)
    with pytest.raises(AssertionError):
        ops.nav_status_reduce(st.sums, st.episode_num, st.rings, torch.zeros(22, dtype=torch.float64))
    with pytest.raises(TypeError):
        st.update(torch.zeros((2, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        st.update(torch.zeros((2, 5), dtype=torch.int32))
    with pytest.raises(ValueError):
        NavStatus(0, "cpu")


def test_state_dict_round_trip_on_host_tensors():
    import torch
    from ddrl4nav_amd.agent import NavStatus
    _, m = model_checkpoints()
    a, b = NavStatus(N, "cpu"), NavStatus(N, "cpu")
    named = a.named_tensors()
    assert tuple(named) == S.PER_ENV
    for name, t in named.items():                                       # the named tensors are views of the three buffers
        t.copy_(torch.from_numpy(getattr(m, name)))
    assert np.array_equal(a.sums.numpy()[5], m.steps_episode) and np.array_equal(a.sums.numpy()[12], m.v_speeds_sum_no_human)
    assert np.array_equal(a.rings.numpy()[4], m.trunc_num) and np.array_equal(a.rings.numpy()[1], m.coll_static_num)
    sd = a.state_dict()
    assert sorted(sd) == ["episode_num", "rings", "sums"] and not any(v.is_cuda for v in sd.values())
    b.load_state_dict(sd)
    for name, t in b.named_tensors().items():
        assert np.array_equal(bits(t.numpy()), bits(getattr(m, name))), name
    for key, wrong in (("sums", torch.zeros((18, N + 1))), ("episode_num", torch.zeros(N)), ("rings", torch.zeros((4, 100, N)))):
        with pytest.raises(ValueError):
            b.load_state_dict(dict(sd, **{key: wrong}))
