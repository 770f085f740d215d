"""The PPO update options on the GPU: the option instantiations of the loss kernels of both head families
against float64 under the yardsticks of tests/test_heads_optim_ops_gpu.py, ddrl_ppo_iter_opt against ddrl_ppo_iter / _indexed bit for
bit where the options are off or cannot matter, the whole Atari context against the float64 oracle, ddrl_set_rates, ddrl_op_gather_f32,
and PPO.learn / GenericPPO.learn with each knob against the C API driven by hand.  Run with `-m gpu`."""
import functools
from ctypes import byref, c_int64

import numpy as np
import pytest
import torch

import config_cross as X
import heads_ref as H
import loss_options_ref as LR
import test_heads_optim_ops_gpu as T
import test_in_place_gpu as IP

pytestmark = pytest.mark.gpu

dev = IP.dev


# ---- 1. ddrl_op_heads_loss_opt against float64 -----------------------------------------------------------------------------------------------
def run_heads_loss_opt(c):
    """test_heads_optim_ops_gpu.run_heads_loss through the option entry point: the same buffers, sentinels and result dict."""
    _lib, lib = T._load()
    L = H.head_layout(c.continuous, c.A)
    d = T._desc(c, L)
    f = dict(dtype=torch.float32, device="cuda")
    params = H.fill_arena(L, c.params, fill=0.5).cuda()
    grads = torch.full((L["n_params"] + 8,), T.SENT, **f)
    wf = c_int64()
    _lib.check(lib.ddrl_op_heads_ws_floats(byref(d), c.n, byref(wf)))
    ws = torch.zeros(wf.value, **f)
    ha, hc = c.ha.cuda(), c.hc.cuda()
    dh_a = torch.full((c.n + 2, H.FEAT), T.SENT, **f)
    dh_c = torch.full((c.n + 2, H.FEAT), T.SENT, **f)
    cfg = T._cfg(c)
    acts, old, adv, ret = (t.contiguous().cuda() for t in (c.actions, c.old_logps, c.advs, c.rets))
    # the fifth column is handed over only where the clip reads it: the entropy-only cases pass NULL
    vold = c.old_values.cuda() if c.value_clip > 0 else None
    opt = _lib.LossOptions(c.value_clip, 1 if c.entropy_split else 0)
    _lib.check(lib.ddrl_op_heads_loss_opt(byref(d), byref(cfg), T._p(params), T._p(ha), T._p(hc), c.n, T._p(acts), T._p(old), T._p(adv),
                                          T._p(ret), byref(opt), T._p(vold), c.B_global, T._p(dh_a), T._p(dh_c), T._p(grads), T._p(ws),
                                          T._st()))
    torch.cuda.synchronize()
    return {"L": L, "dh_actor": dh_a.cpu(), "dh_critic": dh_c.cpu(), "grads": grads.cpu()}


@pytest.mark.parametrize("spec", LR.loss_cases(), ids=LR.case_id)
def test_heads_loss_opt_vs_float64(spec, monkeypatch):
    """check_heads_loss and judge of tests/test_heads_optim_ops_gpu.py as they are; the reference they call is the option restatement."""
    c = LR.case_of(spec)
    LR.check_recipe(c)
    monkeypatch.setattr(T.H, "loss_block", LR.loss_block)
    T.check_heads_loss(c, run_heads_loss_opt(c), LR.case_id(spec))


def test_heads_loss_opt_with_the_options_off_is_heads_loss():
    for cont, A in ((0, 6), (0, 8), (0, 18), (1, 3)):
        c = LR.make_case(cont, A, 67, 0, 1, (0.0, False), seed=2)
        plain, opt = T.run_heads_loss(c), run_heads_loss_opt(c)
        for k in ("dh_actor", "dh_critic", "grads"):
            assert torch.equal(plain[k].view(torch.int32), opt[k].view(torch.int32)), (cont, A, k)


# ---- 2. ddrl_ppo_iter_opt against ddrl_ppo_iter / ddrl_ppo_iter_indexed ------------------------------------------------------------------------
def iter_opt(hp, frames, cols, options, old_values=None, tab=None):
    """ddrl_ppo_iter_opt whatever the options (HotPath.ppo_iter takes the plain entry point when both are off)."""
    B = cols[0].numel()
    hp.loss_options = options
    if tab is None:
        hp._ppo_iter_opt(frames, 0, None, *cols, old_values, B, None)
    else:
        hp._ppo_iter_opt(frames, frames.numel() // (84 * 84), tab, *cols, old_values, B, None)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("shared", [0, 1], ids=["separate", "shared"])
def test_ppo_iter_opt_bit_identities(shared):
    C = 4
    planes, age, _ = IP.pool(C)
    planes_dev = dev(planes)
    hp = IP.make_hot_path(67, C, shared)
    try:
        for B in (1, 2, 3, 4, 5, 6, 7, 67):
            cols = IP.columns(B, 20 * B + shared)
            vold = (cols[3] + 0.3 * dev(np.random.default_rng(B).normal(size=B).astype(np.float32))).contiguous()
            idx = np.random.default_rng(100 + B).integers(0, IP.T * IP.N, size=B).astype(np.int32)
            tab = IP.build(C, "planes", idx=idx)[0].contiguous()
            flat = planes_dev.reshape(-1, 84, 84)
            frames = flat[tab[:, :C].long()].contiguous()
            hp.loss_options = (0.0, False)
            plain = IP.one_iteration(hp, B, cols, lambda: hp.ppo_iter(frames, *cols))
            indexed = IP.one_iteration(hp, B, cols, lambda: hp.ppo_iter_indexed(planes_dev, tab, *cols))
            assert same(plain, indexed)
            # default options through the option entry point: the whole arena, the statistics, a1 and the sign masks, the diagnostics
            assert same(plain, IP.one_iteration(hp, B, cols, lambda: iter_opt(hp, frames, cols, (0.0, False)))), B
            assert same(plain, IP.one_iteration(hp, B, cols, lambda: iter_opt(hp, planes_dev, cols, (0.0, False), tab=tab))), B
            split = IP.one_iteration(hp, B, cols, lambda: iter_opt(hp, frames, cols, (0.0, True)))
            if shared:      # total_loss carries the entropy term already
                assert same(plain, split), B
            else:
                assert not torch.equal(plain[0], split[0])
                n = hp.n_params
                assert torch.equal(plain[0][n:n + 3], split[0][n:n + 3])       # the three statistics are unchanged
            for options in ((0.25, False), (0.0, True), (0.25, True)):
                a = IP.one_iteration(hp, B, cols, lambda: iter_opt(hp, frames, cols, options, vold))
                b = IP.one_iteration(hp, B, cols, lambda: iter_opt(hp, planes_dev, cols, options, vold, tab=tab))
                again = IP.one_iteration(hp, B, cols, lambda: iter_opt(hp, frames, cols, options, vold))
                assert same(a, b) and same(a, again), (B, options)
                if options[0] > 0 and B == 67:
                    assert not torch.equal(a[0], plain[0]), options
    finally:
        hp.close()


def test_entropy_split_with_a_zero_coefficient_changes_no_number():
    from ddrl4nav_amd.engine import HotPath
    C, B = 4, 7
    hp = HotPath(8, n_actions=6, in_channels=C, ent_loss_theta=0.0)
    try:
        g = torch.Generator(device="cpu").manual_seed(5)
        hp.params.copy_(torch.randn(hp.n_params, generator=g) * 0.02)
        hp.params_changed()
        cols = IP.columns(B, 3)
        frames = dev(np.random.default_rng(3).integers(0, 256, size=(B, C, 84, 84), dtype=np.uint8))
        hp.ppo_iter(frames, *cols)
        plain = hp.grads.clone()
        iter_opt(hp, frames, cols, (0.0, True))
        assert bool((hp.grads == plain).all()) and bool(torch.isfinite(plain).all())      # as numbers: a -0.0 equals 0.0
    finally:
        hp.close()


# ---- 3. the whole context against the float64 oracle ----------------------------------------------------------------------------------------------
CELLS = [   # head class x sharing x value loss x option set
    (X.Cell(4, 6, 0, 0, 5, 5), "both"),
    (X.Cell(1, 18, 1, 0, 67, 67), "clip"),
    (X.Cell(3, 8, 0, 1, 33, 33), "entropy"),
    (X.Cell(2, 6, 1, 1, 7, 7), "both"),
    (X.Cell(4, 6, 0, 0, 5, 5), "entropy"),      # every row saturated: ACTOR_BIAS_SHIFT below
]
# Added to the actor bias of action 0 before the weights are flattened.  40: q_0 = 1 to the last bit and every other q_j ~ e^-40 in every
# row, so both clamps of log(clamp(q, eps, 1 - eps)) shut the surrogate's gradient off in float64 and on the device alike; what is left
# on the actor side is the entropy term through log(clamp(q_j)), of order 1e-17.  The checks are those of every other cell.
ACTOR_BIAS_SHIFT = {(X.Cell(4, 6, 0, 0, 5, 5), "entropy"): 40.0}


@pytest.mark.parametrize("cell,name", CELLS, ids=["%s-%s" % (X.cell_id(c), n) for c, n in CELLS])
def test_atari_context_with_options_vs_float64(cell, name):
    from ddrl4nav_amd.engine import HotPath
    from ddrl4nav_amd.utils.recipe import flatten
    import test_config_cross_gpu as G
    frames, acts, old, adv, ret, w = X.cell_inputs(cell)
    if (cell, name) in ACTOR_BIAS_SHIFT:
        w = dict(w)
        w["actor.actor_linear.bias"] = w["actor.actor_linear.bias"].copy()
        w["actor.actor_linear.bias"][0] += ACTOR_BIAS_SHIFT[(cell, name)]
    options = LR.OPTION_SETS[name]
    vold = LR.atari_old_values(cell, w, frames, ret)
    shared = bool(cell.shared)
    hp = HotPath(cell.max_batch, n_actions=cell.A, in_channels=cell.C, share_cnn_net=cell.shared, smooth_l1_loss=cell.smooth_l1)
    try:
        hp.set_params(flatten(w, num_inputs=cell.C, n_actions=cell.A, shared=shared))
        cols = [dev(acts), dev(old), dev(adv), dev(ret)]
        iter_opt(hp, dev(frames), cols, options, dev(vold))
        arena = hp.grads.clone()
        net, losses = LR.atari_oracle64(hp, shared, w, frames, acts, old, adv, ret, vold, bool(cell.smooth_l1), options, n_actions=cell.A,
                                        num_inputs=cell.C)
        flat = arena.cpu().numpy()
        assert np.isfinite(flat).all()
        print("%s %s: losses %s, float64 %s" % (X.cell_id(cell), name, flat[hp.n_params:hp.n_params + 3], losses))
        np.testing.assert_allclose(flat[hp.n_params:hp.n_params + 3], losses, rtol=2e-5, atol=2e-6)
        got = G._split(flat[:hp.n_params], cell)
        failed = []
        for pname, p in net.named_parameters():
            want = p.grad.numpy()
            scale = np.abs(want).max()
            if scale == 0.0:
                assert not got[pname].any(), pname
                continue
            err = np.abs(got[pname] - want).max()
            a, b = got[pname].astype(np.float64).ravel(), want.ravel()
            one_minus_cos = 1.0 - a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
            print("%s %s %s: %.2e max|g64|, 1 - cos %.1e" % (X.cell_id(cell), name, pname, err / scale, one_minus_cos))
            if not (err <= 2e-5 * scale and one_minus_cos < 1e-9):
                failed.append((pname, err / scale, one_minus_cos))
        assert not failed, failed
    finally:
        hp.close()


# ---- 4. ddrl_set_rates ---------------------------------------------------------------------------------------------------------------------------
X_RATES = dict(actor_lr=5e-5, critic_lr=1e-3, learning_rate=2e-4, ppo_clip=0.2)
Y_RATES = dict(actor_lr=3.1e-5, critic_lr=7.7e-4, learning_rate=1.3e-4, ppo_clip=0.13)


@pytest.mark.parametrize("shared", [0, 1], ids=["two_lr", "shared"])
def test_set_rates_equals_a_context_created_with_them(shared):
    from ddrl4nav_amd._lib import check
    from ddrl4nav_amd.engine import HotPath
    B = 5
    a, b = HotPath(8, share_cnn_net=shared, **X_RATES), HotPath(8, share_cnn_net=shared, **Y_RATES)
    try:
        g = torch.Generator(device="cpu").manual_seed(9)
        p0 = torch.randn(a.n_params, generator=g) * 0.02
        grads = torch.randn(a.n_params + 8, generator=g) * 1e-3
        for hp in (a, b):
            hp.params.copy_(p0)
            hp.params_changed()
            hp.grads.copy_(grads)
        a.set_rates(**Y_RATES)
        a.clip_adam_step()
        b.clip_adam_step()
        for k in ("params", "adam_m", "adam_v"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert not torch.equal(a.params.cpu(), p0)
        # ppo_clip reaches the loss kernel and the diagnostics
        cols = IP.columns(B, 4)
        frames = dev(np.random.default_rng(4).integers(0, 256, size=(B, 4, 84, 84), dtype=np.uint8))
        for hp in (a, b):
            hp.params.copy_(p0)
            hp.params_changed()
        out = [IP.one_iteration(hp, B, cols, lambda: hp.ppo_iter(frames, *cols)) for hp in (a, b)]
        assert same(out[0][:2], out[1][:2])
        # refused values leave the context as it was
        before = [x.clone() for x in IP.one_iteration(a, B, cols, lambda: a.ppo_iter(frames, *cols))]
        nan = float("nan")
        for bad in ((-1.0, 1e-3, 2e-4, 0.2), (5e-5, nan, 2e-4, 0.2), (5e-5, 1e-3, float("inf"), 0.2), (5e-5, 1e-3, 2e-4, -0.1)):
            assert a.lib.ddrl_set_rates(a.ctx, *bad) == -1
        assert same(before, IP.one_iteration(a, B, cols, lambda: a.ppo_iter(frames, *cols)))
        a.grads.copy_(grads)
        b.grads.copy_(grads)
        a.clip_adam_step()
        b.clip_adam_step()
        assert torch.equal(a.params, b.params) and a.step == b.step == 2
        check(a.lib.ddrl_set_rates(a.ctx, 0.0, 0.0, 0.0, 0.0))       # zero is a legal rate: the floor of a schedule
        p = a.params.clone()
        a.grads.copy_(grads)
        a.clip_adam_step()
        assert torch.equal(a.params, p)
    finally:
        a.close()
        b.close()


# ---- 5. ddrl_op_gather_f32 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 300])
def test_gather_f32_against_numpy(n):
    from ddrl4nav_amd import ops
    rows = 37
    rng = np.random.default_rng(n)
    src = rng.normal(size=rows).astype(np.float32)
    idx = rng.integers(0, rows, size=n).astype(np.int32)
    hostile = idx.copy()
    hostile[::3] = np.resize(np.array([-1, rows, 2 ** 31 - 1, -2 ** 31, rows + 5], np.int32), len(hostile[::3]))
    sent = -7.5e8
    for ix in (idx, hostile):
        dst = torch.full((n + 3,), sent, dtype=torch.float32, device="cuda")
        out = ops.gather_f32(dev(src), dst, idx=dev(ix), n=n)
        ok = (ix >= 0) & (ix < rows)
        want = np.where(ok, src[np.where(ok, ix, 0)], 0.0).astype(np.float32)
        assert np.array_equal(out.cpu().numpy(), want) and bool((dst[n:] == sent).all())
    for first in (0, 3, rows - 2, -2, rows, 2 ** 40, -2 ** 40):
        dst = torch.full((n + 3,), sent, dtype=torch.float32, device="cuda")
        out = ops.gather_f32(dev(src), dst, first=first, n=n)
        r = first + np.arange(n, dtype=np.int64)
        ok = (r >= 0) & (r < rows)
        want = np.where(ok, src[np.where(ok, r, 0)], 0.0).astype(np.float32)
        assert np.array_equal(out.cpu().numpy(), want) and bool((dst[n:] == sent).all()), first


# ---- 6. PPO.learn with each knob against the C API driven by hand -----------------------------------------------------------------------------------
KNOBS = {"clip": dict(VALUE_CLIP=0.2), "entropy": dict(ENTROPY_BONUS_SPLIT=True), "both": dict(VALUE_CLIP=0.2, ENTROPY_BONUS_SPLIT=True)}
B = LR.N_ENVS * LR.HORIZON


@functools.lru_cache(maxsize=None)
def rollouts(with_old_values):
    """(DeviceRollout, PlaneRollout) of one 8-env x 8-step rollout acted by a net that asks for the collecting policy's values or not;
    never modified afterwards."""
    net = LR.make_net(**(dict(VALUE_CLIP=0.2) if with_old_values else {}))
    a, b = LR.rollout("DeviceRollout", net), LR.rollout("PlaneRollout", net)
    ea, eb = a.batch(), b.batch()
    for k in ("advs", "actions", "old_logps", "values"):
        assert torch.equal(getattr(ea, k), getattr(eb, k)), k
    assert ea.values.shape == ((2, B) if with_old_values else (1, B))
    if with_old_values:
        assert torch.equal(ea.values[1], a.values[:LR.HORIZON].reshape(B)) and torch.equal(ea.values[0], a.ret.view(B))
    return a, b


def state(net):
    hp = net.hot_path
    return [hp.params.clone(), hp.adam_m.clone(), hp.adam_v.clone()]


@pytest.mark.parametrize("mode", ["full-batch", "K2-shuffled"])
@pytest.mark.parametrize("source", ["DeviceRollout", "PlaneRollout"])
@pytest.mark.parametrize("knob", list(KNOBS))
def test_learn_with_a_knob_equals_the_hand_driven_loop(knob, source, mode):
    from ddrl4nav_amd.nn import minibatch as M
    opts = KNOBS[knob]
    a, b = rollouts("VALUE_CLIP" in opts)
    exp = (a if source == "DeviceRollout" else b).batch()
    mb = dict(PPO_MINIBATCHES=2, PPO_SHUFFLE=True) if mode != "full-batch" else {}
    hand = LR.make_net(iters=2)
    before = hand.hot_path.params.clone()
    steps = [torch.arange(B)] * 2
    if mb:
        steps = [M.epoch_order(hand._seed, 0, e, B).long()[lo:hi] for e in range(2) for lo, hi in M.split(B, 2)]
    frames = a.frames[:LR.HORIZON].reshape(B, LR.CH, 84, 84)
    ea = a.batch()
    cols = [ea.actions, ea.old_logps, ea.advs, ea.values[0].contiguous()]
    vold = ea.values[1].contiguous() if "VALUE_CLIP" in opts else None
    want = LR.hand_loop(hand, frames, cols, vold, steps, (opts.get("VALUE_CLIP", 0.0), opts.get("ENTROPY_BONUS_SPLIT", False)))
    plain = LR.hand_loop(LR.make_net(iters=2), frames, cols, None, steps, (0.0, False))
    assert want != plain                                              # the knob did something
    assert not torch.equal(hand.hot_path.params, before)
    for in_place in (False, True):
        net = LR.make_net(iters=2, FRAMES_IN_PLACE=in_place, **opts, **mb)
        assert net._seed == hand._seed
        got = LR.run_learn(net, exp)
        assert got == want, (in_place, got, want)                      # floats compared with ==: the same bits
        assert same(state(net), state(hand)) and net.hot_path.step == hand.hot_path.step == len(want) == (4 if mb else 2)


def test_learn_raises_on_a_batch_without_old_values():
    a, _ = rollouts(False)
    net = LR.make_net(VALUE_CLIP=0.2)
    with pytest.raises(ValueError, match="VALUE_CLIP"):
        next(net.learn(a.batch()))
    assert net.update_time == 0 and net.hot_path.step == 0


@pytest.mark.parametrize("deferred", [False, True], ids=["eager", "deferred"])
def test_annealed_rates_equal_hand_driven_set_rates(deferred):
    a, _ = rollouts(False)
    exp = a.batch()
    N = 4
    net = LR.make_net(iters=3, LR_ANNEAL_UPDATES=N, CLIP_ANNEAL=True, DEFERRED_LOSS_READBACK=deferred)
    hand = LR.make_net(iters=3)
    base = net._base_rates
    assert [float(np.float32(x)) for x in base] == [float(np.float32(x)) for x in (5e-5, 1e-3, 2e-4, 0.2)]
    rates = [LR.annealed_rates32(base, u, N, 0.0, True) for u in range(3)]
    assert rates[0] == [float(np.float32(x)) for x in base] and rates[2][3] == float(np.float32(0.2 * 0.5))
    frames = a.frames[:LR.HORIZON].reshape(B, LR.CH, 84, 84)
    cols = [exp.actions, exp.old_logps, exp.advs, exp.values[0].contiguous()]
    want = LR.hand_loop(hand, frames, cols, None, [torch.arange(B)] * 3, (0.0, False), rates=rates)
    got = LR.run_learn(net, exp)
    assert got == want and same(state(net), state(hand)) and net.anneal_step == 3
    unannealed = LR.hand_loop(LR.make_net(iters=3), frames, cols, None, [torch.arange(B)] * 3, (0.0, False))
    assert unannealed[0] == want[0] and unannealed[2] != want[2]
    # the next call goes on at u = 3; past the end the floor holds
    floor = LR.make_net(iters=2, LR_ANNEAL_UPDATES=1, LR_ANNEAL_FLOOR=0.0)
    p0 = floor.hot_path.params.clone()
    LR.run_learn(floor, exp)
    first = floor.hot_path.params.clone()
    assert not torch.equal(first, p0) and floor.anneal_step == 2
    LR.run_learn(floor, exp)
    assert torch.equal(floor.hot_path.params, first)                    # s = 0 from u = 1 on: the second step of the first call moved nothing either


def test_a_step_skipped_by_target_kl_does_not_advance_the_schedule():
    a, _ = rollouts(False)
    net = LR.make_net(iters=3, LR_ANNEAL_UPDATES=4, TARGET_KL=1e-9)
    exp = a.batch()
    # the batch was collected by the same weights: the first step's KL is rounding noise, the second one's is not
    items = [u for _, u, _ in net.learn(exp)]
    assert len(items) == net.anneal_step == net.hot_path.step < 3


def test_generic_ppo_with_the_knobs_equals_heads_loss_opt_by_hand():
    """The MLP net (classical control, two actions, separate encoders), n = 67, one step."""
    from ddrl4nav_amd import ops
    from ddrl4nav_amd._lib import check
    from ddrl4nav_amd.data import Experience
    from ddrl4nav_amd.ops import _p, _st
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.utils.recipe import hash_weights
    import test_generic_gpu as GG
    n = 67
    rng = np.random.default_rng(67)
    states = rng.normal(size=(n, 4)).astype(np.float32)
    acts = rng.integers(0, 2, size=n).astype(np.float32)
    old = (np.full(n, -np.log(2)) + rng.normal(0, 0.3, n)).astype(np.float32)
    adv, ret = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    vold = (ret + rng.normal(0, 0.5, n)).astype(np.float32)
    options = dict(VALUE_CLIP=0.3, ENTROPY_BONUS_SPLIT=True, LR_ANNEAL_UPDATES=2)

    def make(**opts):
        c = GG._configs({"discrete_action": True, "discrete_actions": [0, 1], "input_dim": 4}, task="classical")
        c["config_nn"].TRAINING_ITER_TIME = 2
        for k, v in opts.items():
            setattr(c["config_nn"], k, v)
        net = create_net(c, max_batch=128)
        w = hash_weights([(k, tuple(p.shape)) for k, p in net.named_parameters()], 15)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
        return net

    net, hand, plain = make(**options), make(), make()
    assert net.loss_options == (0.3, True) and net.wants_old_values and not hand.wants_old_values
    exp = lambda rows: Experience(states=[states], advs=adv, actions=acts, old_logps=old, values=np.stack(rows))
    items = [l for l, _, _ in net.learn(exp([ret, vold]))]
    [l for l, _, _ in plain.learn(exp([ret]))]
    with pytest.raises(ValueError, match="VALUE_CLIP"):
        next(make(**options).learn(exp([ret])))
    d = [dev(x) for x in (acts, old, adv, ret, vold)]
    st = [dev(states)]
    base = hand._base_rates
    for u in range(2):
        c = hand._cfg
        c.actor_lr, c.critic_lr, c.learning_rate, c.ppo_clip = LR.annealed_rates32(base, u, 2)
        hand._ensure_packed()
        ha, hc = hand._features(st, n)
        ops.heads_loss_opt(hand._hd, c, hand.params, ha, hc, n, d[0], d[1], d[2], d[3], (0.3, True), d[4], n, hand._dh[0], hand._dh[1],
                           hand.gtmp, hand._heads_ws)
        hand._backward_both(hand._dh[0], hand._dh[1], n)
        hand.grads.copy_(hand.gtmp)
        hand._step += 1
        check(hand.lib.ddrl_op_clip_adam(byref(c), _p(hand.params), _p(hand.grads), _p(hand.adam_m), _p(hand.adam_v), hand.n_params,
                                         hand.n_actor, 0, hand._step, _p(hand._adam_ws), _st()))
        hand._dirty = True
        s = hand.stats()
        assert all(items[u][k] == s[k] for k in LR.LOSS_KEYS), (u, items[u], s)
    assert torch.equal(net.params, hand.params) and torch.equal(net.adam_v, hand.adam_v) and torch.equal(net.grads, hand.grads)
    assert not torch.equal(net.params, plain.params) and net.anneal_step == 2
