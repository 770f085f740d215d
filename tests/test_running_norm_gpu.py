"""The running observation / return normalisation on the GPU: the five operators of csrc/runnorm.hip, agent.RunningNorm and the
rollouts' knobs against the float64 model of tests/running_norm_ref.py.  Small shapes; the kernels are deterministic, so whatever is
fp32 arithmetic on given fp32 inputs (normalise, discounted returns, GAE) is compared bit for bit, and whatever comes out of double
sums inside the bounds the model states.  Run with `-m gpu`."""
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import running_norm_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON = -7.5e8


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def strided(x, ld, offset=0, fill=POISON):
    """x [n, d] as a device view with row stride ld whose first element lies `offset` floats behind a 256-byte aligned base; returns
    (view, the whole buffer)."""
    n, d = x.shape
    buf = torch.full((offset + n * ld + 4,), fill, dtype=torch.float32, device="cuda")
    view = buf[offset:offset + n * ld].view(n, ld)[:, :d]
    view.copy_(dev(x))
    return view, buf


# ---- 1. column moments -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.MOMENT_SHAPES)
def test_column_moments_against_the_two_pass_model(shape):
    from ddrl4nav_amd import ops
    n, d, ld = shape
    x = R.columns(np.random.default_rng(n * 131 + d), n, d, ld)          # NaN in the padding columns: read = seen
    mean64, var64 = R.two_pass(x[:, :d])
    e_mean, e_var = R.moments_bound(n, mean64, var64)
    xd = dev(x)
    view = xd if ld == d else xd[:, :d]
    sums = ops.column_moments(view, d)
    got = host(sums)
    assert got.shape == (1 + 2 * d,) and got[0] == n and np.isfinite(got).all()
    mean, var = R.moments_of_sums(got, d)
    print("n %d d %d ld %d: mean err / bound %.3g, var err / bound %.3g" % (n, d, ld, np.max(np.abs(mean - mean64) / np.maximum(e_mean, 1e-300)),
                                                                            np.max(np.abs(var - var64) / np.maximum(e_var, 1e-300))))
    assert np.all(np.abs(mean - mean64) <= e_mean) and np.all(np.abs(var - var64) <= e_var)
    # a repeat gives the same bits; so does a base pointer one float off 16-byte alignment (the scalar path)
    assert np.array_equal(host(ops.column_moments(view, d)), got)
    off_view, _ = strided(x[:, :d], ld, offset=1)
    assert off_view.data_ptr() % 16 == 4
    assert np.array_equal(host(ops.column_moments(off_view, d)), got)
    if ld % 4 == 0:      # ... and a row stride that rules the 16-byte loads out
        odd_view, _ = strided(x[:, :d], ld + 1)
        assert np.array_equal(host(ops.column_moments(odd_view, d)), got)
    # accumulate: added to what the sums hold (here: themselves, and a sentinel row)
    twice = ops.column_moments(view, d, sums=sums.clone(), accumulate=True)
    assert np.array_equal(host(twice), got + got)
    over = ops.column_moments(view, d, sums=torch.full_like(sums, 1e30), accumulate=False)
    assert np.array_equal(host(over), got)


def test_column_moments_workspace_is_what_the_query_says():
    """The slabs' rows fill ws to the last double and nothing behind it."""
    from ddrl4nav_amd import ops
    n, d = 37, 9
    x = dev(R.columns(np.random.default_rng(5), n, d))
    need = ops.column_moments_ws_floats(n, d)
    ws = torch.full((need + 64,), POISON, dtype=torch.float32, device="cuda")
    ops.column_moments(x, d, ws=ws[:need])
    assert torch.all(ws[need:] == POISON) and not torch.any((ws[:need].view(-1, 2) == POISON).all(dim=1))


# ---- 2. merge ------------------------------------------------------------------------------------------------------------------------------
def _check_state(got, want_run, bm=None, bv=None, prior=None):
    d = len(want_run.mean)
    assert got[0] == want_run.count
    mean, var = got[1:1 + d], got[1 + d:]
    bm = np.zeros(d) if bm is None else bm
    bv = np.zeros(d) if bv is None else bv
    delta = np.zeros(d) if prior is None else bm - prior.mean
    assert np.all(np.abs(mean - want_run.mean) <= 1e-14 * (np.abs(want_run.mean) + np.abs(bm)))
    assert np.all(np.abs(var - want_run.var) <= 1e-14 * (want_run.var + bv + delta ** 2))


def test_running_merge_against_the_model():
    """Given the same sums the state equals the model's: the first update from count = 0, n = 1, a constant column, an empty batch,
    then batches on top of one another."""
    from ddrl4nav_amd import ops
    rng = np.random.default_rng(11)
    d = 5
    state = ops.running_state(d, "cuda")
    run = R.RunningRef(d)
    assert np.array_equal(host(state), run.state())
    batches = [np.zeros((0, d)), R.columns(rng, 1, d), np.zeros((0, d)), R.columns(rng, 7, d), R.columns(rng, 513, d)]
    batches[3][:, 2] = 4.25                                      # a constant column: bv = 0
    for x in batches:
        sums = R.sums64(x) if len(x) else np.concatenate([[0.0], rng.normal(size=2 * d)])      # n = 0: the rest is never looked at
        prior = run.copy()
        before = host(state).copy()
        sd = dev(sums)
        ops.running_merge(sd, state)
        assert np.array_equal(host(sd), sums)                    # the sums are not modified
        if len(x) == 0:
            assert np.array_equal(host(state), before)
            continue
        run.merge_sums(sums)
        bm = sums[1:1 + d] / len(x)
        bv = np.maximum(0.0, sums[1 + d:] / len(x) - bm * bm)
        _check_state(host(state), run, bm, bv, prior)
    assert host(state)[0] == 521
    assert host(state)[1 + d + 2] >= 0


def test_running_merge_reproduces_the_reference_fixture(golden):
    """Fixture f28 end to end on the device: column_moments of each batch, merge; against the reference's own RunningMeanStd."""
    from ddrl4nav_amd import ops
    g = golden("f28_running_mean_std")
    state = ops.running_state(5, "cuda")
    ref = R.BoundedRef(5)
    for i, n in enumerate(g["batches"]):
        x = g["x%d" % i]
        ops.running_merge(ops.column_moments(dev(x.astype(np.float32)), 5), state)
        ref.update(x)
        ref.check(host(state), ref=np.concatenate([[g["count%d" % (i + 1)]], g["mean%d" % (i + 1)], g["var%d" % (i + 1)]]))


# ---- 3. affine and normalise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("center", [True, False])
def test_running_affine(center):
    """shift is the mean rounded to fp32 (0 without center); scale is one fp32 rounding of a double 1 / sqrt(var + eps): at most one fp32
    ulp from the model's, whose double square root and division may differ from the device's in the last place."""
    from ddrl4nav_amd import ops
    rng = np.random.default_rng(3)
    d = 37
    mean, var = rng.normal(size=d) * 10.0 ** rng.uniform(-3, 3, size=d), 10.0 ** rng.uniform(-6, 6, size=d)
    var[:3] = (0.0, 1.0, 4.0)
    for eps in (0.0, 1e-8, 1e-2):
        if eps == 0.0:
            var[0] = 0.25
        state = dev(np.concatenate([[12.0], mean, var]))
        aff = host(ops.running_affine(state, eps, center=center))
        want = R.affine_ref(mean, var, eps, center)
        assert aff.shape == (2, d) and np.array_equal(aff[0], want[0])
        assert np.all(np.abs(aff[1].astype(np.float64) - want[1]) <= 2.0 ** -23 * want[1])
        if eps == 0.0:
            assert np.array_equal(aff[1][:3], [2.0, 1.0, 0.5])                   # exact roots and quotients
    if not center:
        assert not aff[0].any()


def _norm_case(rng, n, d):
    x = R.columns(rng, n, d)
    aff = R.affine_ref(x.mean(axis=0, dtype=np.float64), x.var(axis=0, dtype=np.float64), 1e-8)
    return x, aff


@pytest.mark.parametrize("n,d,ld_x,ld_out", [(1, 1, 1, 1), (7, 5, 5, 5), (513, 3, 8, 8), (33, 960, 960, 964), (19, 257, 259, 257), (300, 1, 1, 1),
                                             (5, 6912, 6912, 6912), (9, 1025, 1028, 1032)])
def test_normalize_columns_bit_exact(n, d, ld_x, ld_out):
    from ddrl4nav_amd import ops
    rng = np.random.default_rng(n + d)
    x, aff = _norm_case(rng, n, d)
    flat = x.reshape(-1)
    flat[rng.integers(0, flat.size, size=min(6, flat.size))] = (np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 0.0)[:min(6, flat.size)]
    affd = dev(aff)
    for clip in (10.0, 0.5, float("inf")):
        want = R.normalize_ref(x, aff, clip)
        xv, _ = strided(x, ld_x)
        ov, obuf = strided(np.zeros_like(x), ld_out)
        ov.fill_(POISON - 1)
        before = obuf.clone()
        ops.normalize_columns(xv, affd, clip, out=ov)
        assert np.array_equal(host(ov), want, equal_nan=True), clip
        mask = torch.ones_like(obuf, dtype=torch.bool)
        mask[:n * ld_out].view(n, ld_out)[:, :d] = False
        assert torch.equal(obuf[mask], before[mask])                         # padding columns and the tail are never written
        ops.normalize_columns(xv, affd, clip, out=xv)                       # in place
        assert np.array_equal(host(xv), want, equal_nan=True)
        off, _ = strided(x, ld_x, offset=3)                                 # the scalar path gives the same bits
        assert np.array_equal(host(ops.normalize_columns(off, affd, clip)), want, equal_nan=True)


def test_normalize_columns_edges():
    """Values landing exactly on +-clip, infinities to +-clip, NaN stays NaN, clip = inf, center = 0."""
    from ddrl4nav_amd import ops
    aff = np.array([[1.0, 0.0, -2.0], [0.5, 2.0, 1.0]], np.float32)
    x = np.array([[21.0, 5.0, 8.0], [-19.0, -5.0, -12.0], [np.inf, -np.inf, np.nan], [21.000002, 4.9999995, -12.000001],
                  [np.nan, np.inf, -np.inf], [1.0, 0.0, -2.0]], np.float32)
    got = host(ops.normalize_columns(dev(x), dev(aff), 10.0))
    assert np.array_equal(got[:2], [[10.0, 10.0, 10.0], [-10.0, -10.0, -10.0]])
    assert np.array_equal(got[2][:2], [10.0, -10.0]) and np.isnan(got[2][2])
    assert got[3][0] == 10.0 and got[3][1] < 10.0 and got[3][2] == -10.0
    assert np.isnan(got[4][0]) and np.array_equal(got[4][1:], [10.0, -10.0]) and not got[5].any()
    assert np.array_equal(got, R.normalize_ref(x, aff, 10.0), equal_nan=True)
    wide = host(ops.normalize_columns(dev(x), dev(aff), float("inf")))
    assert np.array_equal(wide, R.normalize_ref(x, aff, np.inf), equal_nan=True) and wide[2][0] == np.inf and wide[0][0] == 10.0
    # center = 0 through the operators: the state's mean is not subtracted
    state = dev(np.array([9.0, 7.0, -3.0, 4.0, 0.25]))
    a0 = ops.running_affine(state, 0.0, center=False)
    y = host(ops.normalize_columns(dev(np.array([[2.0, 1.0], [-4.0, 100.0]], np.float32)), a0, 10.0))
    assert np.array_equal(y, [[1.0, 2.0], [-2.0, 10.0]])


# ---- 4. discounted returns -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65])
@pytest.mark.parametrize("T", [1, 9])
def test_discounted_returns_bit_exact(N, T):
    from ddrl4nav_amd import ops
    rng = np.random.default_rng(N * 10 + T)
    r = (rng.normal(size=(T, N)) * 10).astype(np.float32)
    d = (rng.random((T, N)) < 0.2).astype(np.uint8)
    d[0, 0] = 1                                  # a done at t = 0, at T - 1, back to back
    d[T - 1, N - 1] = 1
    if T > 4:
        d[3:5, N // 2] = 1
    carry0 = rng.normal(size=N).astype(np.float32)
    gamma = 0.99
    want, want_carry = R.discounted_ref(r, d, gamma, carry0)
    carry = dev(carry0)
    got = ops.discounted_returns(dev(r), dev(d), gamma, carry)
    assert np.array_equal(host(got), want) and np.array_equal(host(carry), want_carry)
    assert want_carry[N - 1] == 0.0
    if T > 1:                                    # two chained calls equal one call on the concatenation
        carry = dev(carry0)
        k = T // 2
        a = ops.discounted_returns(dev(r[:k]), dev(d[:k]), gamma, carry)
        b = ops.discounted_returns(dev(r[k:]), dev(d[k:]), gamma, carry)
        assert np.array_equal(np.concatenate([host(a), host(b)]), want) and np.array_equal(host(carry), want_carry)


# ---- 5. StateRollout -----------------------------------------------------------------------------------------------------------------------
SN, ST = 3, 4


def _mlp_net():
    """The classical-control net of create_net: MLPPreNet(4, 512) encoders, two actions, hashed weights."""
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.utils.recipe import hash_weights
    env = {"discrete_action": True, "discrete_actions": [0, 1], "input_dim": 4}
    cfg = BaseConfig(types.SimpleNamespace(task="test", ip="127.0.0.1"), dict(env, env_type="gym", env_name="CartPole-v1", env_num=8))
    cfg.TASK_TYPE = "classical"
    cfg_nn = ConfigNN(env)
    cfg_nn.SHARE_CNN_NET = False
    net = create_net({"config": cfg, "config_nn": cfg_nn, "config_env": env}, max_batch=16)
    w = hash_weights([(k, tuple(p.shape)) for k, p in net.named_parameters()], 15)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    return net


def _state_sequence():
    """Two chained rollouts: raw observations [2, T + 1, N, 4] in physical units (offsets and scales that differ by column), rewards of
    order ten, dones."""
    rng = np.random.default_rng(66)
    obs = (np.array([0.0, 30.0, -4.0, 0.5]) + np.array([1.0, 12.0, 0.1, 5.0]) * rng.normal(size=(2, ST + 1, SN, 4))).astype(np.float32)
    rew = (10.0 * rng.normal(size=(2, ST + 1, SN))).astype(np.float32)
    done = (rng.random((2, ST + 1, SN)) < 0.3).astype(np.uint8)
    return obs, rew, done


def _drive(ro, r, obs, rew, done):
    """Rollout r of the sequence: puts (slot 0 of rollout 1 is carried over), act, record, bootstrap, finish.  The net draws its actions
    from a counter-based stream indexed by its forward calls: the counter is set, so that two rollouts driven alike sample alike."""
    ro.net._calls = 100 * (r + 1)
    for t in range(ST + 1):
        if t >= 1 or r == 0:
            ro.put_states(t, [dev(obs[r, t])])
        if t < ST:
            ro.act(t)
            ro.record(t, dev(rew[r, t]), dev(done[r, t]))
    ro.bootstrap()
    ro.finish()


def _snapshot(ro):
    return {k: v.clone() for k, v in dict(states=ro.states[0], values=ro.values, rewards=ro.rewards, dones=ro.dones, actions=ro.actions,
                                          logps=ro.logps, adv=ro.adv, ret=ro.ret).items()}


def test_state_rollout_matches_the_host_replay():
    from ddrl4nav_amd.agent import StateRollout, gae_device
    net = _mlp_net()
    obs, rew, done = _state_sequence()
    ro = StateRollout(net, SN, [(4,)], horizon=ST, track_returns=True, normalize_obs=True, normalize_returns=True, obs_clip=2.5)
    plain = StateRollout(net, SN, [(4,)], horizon=ST, track_returns=True)
    om, rm = R.ObsNormRef(4, clip=2.5), R.ReturnNormRef(SN, 0.99)
    ref, ret_ref = R.BoundedRef(4), R.BoundedRef(1)
    assert ro.obs_norm is not None and len(ro.obs_norm) == 1 and ro.rewards_norm.shape == (ST, SN)
    for r in range(2):
        affine = host(ro.obs_norm[0].affine).copy()                  # as frozen at the last finish(): the fresh state's at first
        assert np.array_equal(affine[0], om.affine[0]) and np.all(np.abs(affine[1] - om.affine[1]) <= 2.0 ** -23 * om.affine[1])
        carried = host(ro.states[0][0]).copy()
        _drive(ro, r, obs, rew, done)
        _drive(plain, r, obs, rew, done)
        # the pool: every put slot is the raw rows normalised with the frozen affine, bit for bit; a carried slot moved as it was
        first = 0 if r == 0 else 1
        for t in range(first, ST + 1):
            assert np.array_equal(host(ro.states[0][t]), R.normalize_ref(obs[r, t], affine, 2.5)), (r, t)
            om.put(obs[r, t])
        if r == 1:
            assert np.array_equal(host(ro.states[0][0]), carried)
        assert np.abs(host(ro.states[0])).max() <= 2.5 and (np.abs(host(ro.states[0])) == 2.5).any()
        # the statistics: the raw rows of the put slots, each counted once, against the reference's update on them
        om.finish()
        ref.update(obs[r, first:].reshape(-1, 4))
        st = host(ro.obs_norm[0].state)
        assert st[0] == (ST + 1) * SN + r * ST * SN
        ref.check(st)
        ref.check(st, factor=2.0, ref=om.run.state())                # the replay's own double sums lie inside the bound too
        # the returns: the discounted-return trace bit for bit, its running variance inside the bounds, rewards_norm bit for bit given
        # the device's own affine, and GAE on exactly those
        raw_r, raw_d = host(ro.rewards), host(ro.dones)
        assert np.array_equal(raw_r, host(plain.rewards)) and np.array_equal(raw_r[first:], rew[r, first:ST])
        carry_before = rm.carry.copy()
        rm.scale(raw_r, raw_d)
        trace, carry = R.discounted_ref(raw_r, raw_d, 0.99, carry_before)
        assert np.array_equal(host(ro.ret_norm.trace), trace) and np.array_equal(host(ro.ret_norm.carry), carry)
        rs = host(ro.ret_norm.norm.state)
        assert rs[0] == (r + 1) * ST * SN
        ret_ref.update(trace.reshape(-1, 1))
        ret_ref.check(rs)
        ret_ref.check(rs, factor=2.0, ref=rm.norm.run.state())
        ra = host(ro.ret_norm.norm.affine)
        assert ra[0][0] == 0.0 and abs(ra[1][0] - rm.norm.affine[1][0]) <= 2.0 ** -23 * rm.norm.affine[1][0]
        assert np.array_equal(host(ro.rewards_norm), R.normalize_ref(raw_r.reshape(-1, 1), ra, 10.0).reshape(ST, SN))
        adv, ret = gae_device(ro.values, ro.rewards_norm, ro.dones, 0.99, 0.95)
        assert torch.equal(adv, ro.adv) and torch.equal(ret, ro.ret)
        assert not torch.equal(ro.adv, plain.adv)
        # the raw rewards and the episode returns are those of a rollout without the knobs
        assert torch.equal(ro.returns.rewards_episode, plain.returns.rewards_episode)
        assert torch.equal(ro.returns.rewards_sum, plain.returns.rewards_sum)
        batch = ro.batch()
        assert batch.states[0].data_ptr() == ro.states[0].data_ptr()          # still zero-copy
        ro.carry_over()
        plain.carry_over()


def test_state_rollout_knobs_off_is_the_rollout_of_before():
    from ddrl4nav_amd.agent import StateRollout
    net = _mlp_net()
    obs, rew, done = _state_sequence()
    a = StateRollout(net, SN, [(4,)], horizon=ST)
    b = StateRollout(net, SN, [(4,)], horizon=ST, normalize_obs=None, obs_clip=10.0, normalize_returns=False, reward_clip=10.0, norm_eps=1e-8)
    c = StateRollout(net, SN, [(4,)], horizon=ST, normalize_obs=[False])
    for ro in (a, b, c):
        assert ro.obs_norm is None and ro.ret_norm is None and ro.rewards_norm is None
        assert ro.state_dict() == {"ret_norm": None, "obs_norm": None}
    snaps = []
    for ro in (a, b, c):
        for r in range(2):
            _drive(ro, r, obs, rew, done)
            ro.carry_over()
        snaps.append(_snapshot(ro))
    for s in snaps[1:]:
        for k, v in snaps[0].items():
            assert torch.equal(v, s[k]), k
    assert np.array_equal(host(a.states[0][1:]), obs[1, 1:])                     # raw, as stored


def test_state_rollout_state_dict_round_trip_continues_bit_identically():
    from ddrl4nav_amd.agent import StateRollout
    net = _mlp_net()
    obs, rew, done = _state_sequence()
    kw = dict(horizon=ST, normalize_obs=[True], normalize_returns=True, obs_clip=3.0, reward_clip=5.0, norm_eps=1e-6)
    a = StateRollout(net, SN, [(4,)], **kw)
    _drive(a, 0, obs, rew, done)
    a.carry_over()
    sd = a.state_dict()
    assert sd["obs_norm"][0]["mean"].dtype == torch.float64 and not sd["obs_norm"][0]["mean"].is_cuda and sd["obs_norm"][0]["clip"] == 3.0
    assert sd["ret_norm"]["norm"]["center"] is False and sd["ret_norm"]["carry"].shape == (SN,)
    b = StateRollout(net, SN, [(4,)], **kw)
    b.load_state_dict(sd)
    b.states[0][0].copy_(a.states[0][0])                                      # the carried slot is pool content, not statistics
    assert torch.equal(b.obs_norm[0].affine, a.obs_norm[0].affine) and torch.equal(b.obs_norm[0].state, a.obs_norm[0].state)
    for ro in (a, b):
        _drive(ro, 1, obs, rew, done)
    sa, sb = _snapshot(a), _snapshot(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.rewards_norm, b.rewards_norm) and torch.equal(a.ret_norm.carry, b.ret_norm.carry)
    assert torch.equal(a.obs_norm[0].state, b.obs_norm[0].state) and torch.equal(a.ret_norm.norm.state, b.ret_norm.norm.state)
    with pytest.raises(ValueError):
        StateRollout(net, SN, [(4,)], horizon=ST).load_state_dict(sd)


def test_ring_fed_puts_count_and_normalise_like_direct_puts():
    """put_state_from_ring against put_states on the same rows, two chained rollouts: component 0 normalised, component 1 left raw (one
    flag per component).  Pools, pending sums, statistics and affine are the same bits."""
    from ddrl4nav_amd.agent import StateRollout
    from ddrl4nav_amd.data import PinnedRing
    N, T, shapes = 5, 3, [(4,), (2, 3)]
    net = types.SimpleNamespace(device=torch.device("cuda:%d" % torch.cuda.current_device()), n_actions=2, continuous=False)
    rng = np.random.default_rng(9)
    obs = [(np.array([0.0, 30.0, -4.0, 0.5]) + np.array([1.0, 12.0, 0.1, 5.0]) * rng.normal(size=(2, T + 1, N, 4))).astype(np.float32),
           (7.0 * rng.normal(size=(2, T + 1, N, 2, 3))).astype(np.float32)]
    kw = dict(horizon=T, normalize_obs=[True, False], obs_clip=2.0)
    direct, fed = StateRollout(net, N, shapes, **kw), StateRollout(net, N, shapes, **kw)
    assert fed.obs_norm[1] is None and fed.obs_norm[0].shape == (4,)
    rings = [PinnedRing(N * 4 * 4, n_slots=8), PinnedRing(N * 6 * 4, n_slots=8)]
    for r in range(2):
        first = 0 if r == 0 else 1
        for t in range(first, T + 1):
            for k, ring in enumerate(rings):
                ring.acquire(timeout_ms=1000)[:] = obs[k][r, t].reshape(-1).view(np.uint8)
                ring.commit()
        for t in range(first, T + 1):
            direct.put_states(t, [dev(o[r, t]) for o in obs])
            for k, ring in enumerate(rings):
                fed.put_state_from_ring(t, k, ring)
        assert torch.equal(fed.obs_norm[0].sums, direct.obs_norm[0].sums) and host(fed.obs_norm[0].sums)[0] == (T + 1 - first) * N
        for ro in (direct, fed):
            ro.finish()
        for k in range(2):
            assert torch.equal(fed.states[k], direct.states[k]), (r, k)
        assert np.array_equal(host(fed.states[1][first:]), obs[1][r, first:])              # the raw component, as it arrived
        assert np.abs(host(fed.states[0])).max() == 2.0
        assert torch.equal(fed.obs_norm[0].state, direct.obs_norm[0].state) and torch.equal(fed.obs_norm[0].affine, direct.obs_norm[0].affine)
        for ro in (direct, fed):
            ro.carry_over()
    assert host(fed.obs_norm[0].state)[0] == (2 * T + 1) * N


# ---- 6. DeviceRollout / PlaneRollout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["device", "plane"])
def test_frame_rollouts_normalize_returns(kind):
    """normalize_returns at N = 2, T = 3 over two chained rollouts, the second after carry_over(keep_step=True): rows 0..T-1 are every
    step exactly once."""
    from ddrl4nav_amd.agent import DeviceRollout, PlaneRollout, gae_device
    N, T = 2, 3
    net = types.SimpleNamespace(device=torch.device("cuda:%d" % torch.cuda.current_device()), n_actions=6)
    cls = DeviceRollout if kind == "device" else PlaneRollout
    ro = cls(net, N, horizon=T, channels=2, track_returns=True, normalize_returns=True, reward_clip=0.5)
    plain = cls(net, N, horizon=T, channels=2, track_returns=True)
    assert plain.ret_norm is None and plain.rewards_norm is None and plain.state_dict() == {"ret_norm": None}
    rng = np.random.default_rng(8)
    rew = (10.0 * rng.normal(size=(2, T + 1, N))).astype(np.float32)
    rew[0, 1, 1] = rew[1, 1, 0] = 1000.0          # one reward per rollout that the clip catches whatever the variance
    done = np.zeros((2, T + 1, N), np.uint8)
    done[0, 1, 0] = done[0, T, 1] = done[1, 2, 1] = 1
    rm, ret_ref = R.ReturnNormRef(N, 0.99, clip=0.5), R.BoundedRef(1)
    for r in range(2):
        for x in (ro, plain):
            x.values.copy_(dev(rng.normal(size=(T + 1, N)).astype(np.float32)) if x is ro else ro.values)
            for t in range(x.t0, T + 1):
                x.record(t, dev(rew[r, t]), dev(done[r, t]))
            x.finish()
        raw_r, raw_d = host(ro.rewards), host(ro.dones)
        assert np.array_equal(raw_r, host(plain.rewards))
        if r == 1:
            assert np.array_equal(raw_r[0], rew[0, T]) and np.array_equal(raw_d[0], done[0, T])     # the kept step
        carry_before = rm.carry.copy()
        rm.scale(raw_r, raw_d)
        trace, carry = R.discounted_ref(raw_r, raw_d, 0.99, carry_before)
        assert np.array_equal(host(ro.ret_norm.trace), trace) and np.array_equal(host(ro.ret_norm.carry), carry)
        rs = host(ro.ret_norm.norm.state)
        assert rs[0] == (r + 1) * T * N
        ret_ref.update(trace.reshape(-1, 1))
        ret_ref.check(rs)
        ret_ref.check(rs, factor=2.0, ref=rm.norm.run.state())
        ra = host(ro.ret_norm.norm.affine)
        assert np.array_equal(host(ro.rewards_norm), R.normalize_ref(raw_r.reshape(-1, 1), ra, 0.5).reshape(T, N))
        assert np.abs(host(ro.rewards_norm)).max() == 0.5
        adv, ret = gae_device(ro.values, ro.rewards_norm, ro.dones, 0.99, 0.95)
        assert torch.equal(adv, ro.adv) and torch.equal(ret, ro.ret) and not torch.equal(ro.adv, plain.adv)
        assert torch.equal(ro.returns.rewards_episode, plain.returns.rewards_episode)
        ro.carry_over(keep_step=True)
        plain.carry_over(keep_step=True)
    fresh = cls(net, N, horizon=T, channels=2, normalize_returns=True, reward_clip=0.5)
    fresh.load_state_dict(ro.state_dict())
    assert torch.equal(fresh.ret_norm.norm.state, ro.ret_norm.norm.state) and torch.equal(fresh.ret_norm.carry, ro.ret_norm.carry)
    assert torch.equal(fresh.ret_norm.norm.affine, ro.ret_norm.norm.affine)


# ---- 7. two ranks --------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_end_with_one_state(tmp_path):
    """Two rounds on two gloo ranks sharing the GPU, shards of 300 and 213 rows, then of 65 rows and none (a rank that commits with
    nothing pending): both ranks merge the same all-reduced sums, so their states are bit-identical; a single process fed the union
    holds the same state inside the moments bound (its sums are folded in another order)."""
    from ddrl4nav_amd.agent import RunningNorm
    rng = np.random.default_rng(21)
    rounds = [R.columns(rng, 513, 5), R.columns(rng, 65, 5)]
    np.savez(tmp_path / "rows.npz", round0=rounds[0], round1=rounds[1])
    port = _free_port()
    procs = []
    bounds = "0,300,513"
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   DDRL_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "running_norm_worker.py"), str(tmp_path),
                                       str(tmp_path / "rows.npz"), bounds], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True))
    try:
        for r, p in enumerate(procs):      # the first failure ends the test (and the other rank)
            out, _ = p.communicate(timeout=300)
            assert p.returncode == 0, "rank %d failed (%d):\n%s" % (r, p.returncode, out[-3000:])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(2))
    assert np.array_equal(r0["state"], r1["state"]) and np.array_equal(r0["affine"], r1["affine"])
    one, ref = RunningNorm((5,), "cuda"), R.BoundedRef(5)
    for x in rounds:
        one.update(dev(x))
        one.commit()
        ref.update(x)
    got, single = r0["state"], host(one.state)
    assert got[0] == single[0] == 578
    ref.check(got)
    ref.check(single)
    ref.check(got, factor=2.0, ref=single)      # each lies within the bound of the reference's update: within twice of one another
