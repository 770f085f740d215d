"""The protocol of GenericPPO.learn (nn/generic.py) over micro-batches: PPO_DIAGNOSTICS leaves the update alone, TARGET_KL stops in
front of the step that went too far and leaves update_time / anneal_step / _step where they were, the annealed rates run on across
learn() calls, and an extra critic on a shared net (PPO.add_critic, the GAIL generator's shape) adds its value loss and its encoder
gradient.  Two nets: the MLP net with a categorical head (n = 67 in micro-batches of 32, 32 and 3) and NavPreNet1D x2 with a Gaussian
head (n = 37 in micro-batches of 16, 16 and 5).  Inputs: tests/generic_cross.py:cell_inputs."""
from ctypes import byref

import numpy as np
import pytest
import torch

import generic_cross as X
import loss_options_ref as LR
import test_generic_cross_gpu as GX
from test_ppo_diag_gpu import DIAG_KEYS, TODAY_KEYS, _target_between

pytestmark = pytest.mark.gpu

LOOP_CELLS = [X.Cell("mlp_split", "cat5", 0, "default", "none", 0, 67, 32), X.Cell("nav1d_split", "gauss2", 0, "default", "none", 0, 37, 16)]
LOSS_KEYS = GX.LOSS_KEYS
both_nets = pytest.mark.parametrize("cell", LOOP_CELLS, ids=X.cell_id)


def _state(net):
    return [t.clone() for t in (net.params, net.adam_m, net.adam_v, net.grads)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _run(net, exp):
    """[(item, update_time, state after the yield)] of one learn() call."""
    out = []
    for ld, ut, last in net.learn(exp):
        assert last is True
        out.append((dict(ld), ut, _state(net)))
    return out


def _exp(cell, old_logps=None, rows=None):
    from ddrl4nav_amd.data import Experience
    x = X.cell_inputs(cell)
    return Experience(states=[s.copy() for s in x.states], advs=x.advs.copy(), actions=x.actions.copy(),
                      old_logps=(x.old_logps if old_logps is None else old_logps).copy(), values=np.stack(rows or [x.rets]))


@both_nets
def test_diagnostics_change_nothing(cell):
    runs = {}
    for on in (False, True):
        net = GX.make_net(cell, TRAINING_ITER_TIME=3, **({"PPO_DIAGNOSTICS": True} if on else {}))
        runs[on] = _run(net, _exp(cell))
    assert len(runs[True]) == len(runs[False]) == 3
    for (a, ua, sa), (b, ub, sb) in zip(runs[True], runs[False]):
        assert set(b) == TODAY_KEYS and set(a) == TODAY_KEYS | set(DIAG_KEYS) and ua == ub
        assert all(a[k] == b[k] for k in LOSS_KEYS)
        assert _same(sa, sb)                 # parameters, both moments and the gradient arena with its statistics tail: bit-identical
        assert all(np.isfinite(a[k]) for k in DIAG_KEYS) and 0.0 <= a["ClipFraction"] <= 1.0 and a["ApproxKL"] >= 0.0 and a["RatioMax"] > 0.0
    assert not _same(runs[True][0][2][:1], runs[True][2][2][:1])


@both_nets
def test_target_kl_stops_before_the_step_that_went_too_far(cell):
    x = X.cell_inputs(cell)
    own = x.logp64.astype(np.float32)           # the collecting policy is the net itself: the first KL is rounding noise, the steps raise it
    exp = lambda: _exp(cell, old_logps=own)
    ANNEAL = dict(LR_ANNEAL_UPDATES=8)
    for lr_scale in (1.0, 10.0, 100.0):
        rates = dict(ACTOR_LEARNING_RATE=5e-5 * lr_scale)
        on = _run(GX.make_net(cell, TRAINING_ITER_TIME=4, PPO_DIAGNOSTICS=True, **ANNEAL, **rates), exp())
        kl = [it["ApproxKL"] for it, _, _ in on]
        ks = [k for k in range(1, len(kl)) if kl[k - 1] > 0 and kl[k] >= 4 * kl[k - 1]]
        if ks:
            break
    else:
        raise AssertionError("no fourfold KL step at any learning rate: %r" % (kl,))
    k = ks[0]
    target = _target_between(kl, k)
    assert max(kl[:k]) <= 1.5 * target < kl[k]
    net = GX.make_net(cell, TRAINING_ITER_TIME=4, TARGET_KL=target, **ANNEAL, **rates)
    run = _run(net, exp())
    assert len(run) == k and [ut for _, ut, _ in run] == list(range(1, k + 1))          # exactly k items, then the generator ends
    assert [it["ApproxKL"] for it, _, _ in run] == kl[:k] and set(run[0][0]) == TODAY_KEYS | set(DIAG_KEYS)
    assert net.update_time == net.anneal_step == net._step == k
    # iteration k + 1 was evaluated, not applied: parameters and both moments of a run of k iterations (the gradient arena holds the
    # evaluated, unapplied gradient of iteration k + 1)
    short = GX.make_net(cell, TRAINING_ITER_TIME=k, PPO_DIAGNOSTICS=True, **ANNEAL, **rates)
    short_run = _run(short, exp())
    assert len(short_run) == k and _same(_state(net)[:3], _state(short)[:3]) and _same(_state(net)[:3], on[k - 1][2][:3])
    # a following call anneals from u = k
    for n2 in (net, short):
        n2.target_kl, n2.training_iter_time = None, 1
        assert len(_run(n2, exp())) == 1
    assert net.anneal_step == short.anneal_step == k + 1 and _same(_state(net), _state(short))
    again = GX.make_net(cell, TRAINING_ITER_TIME=k, PPO_DIAGNOSTICS=True, **ANNEAL, **rates)
    _run(again, exp())
    again.anneal_step, again.training_iter_time = 0, 1            # the schedule set back: another rate, other parameters
    _run(again, exp())
    assert not torch.equal(again.params, net.params)


@both_nets
def test_annealed_rates_over_two_learn_calls_equal_the_hand_driven_loop(cell):
    """LR_ANNEAL_UPDATES + CLIP_ANNEAL + LR_ANNEAL_FLOOR with VALUE_CLIP and ENTROPY_BONUS_SPLIT on three micro-batches, two learn() calls
    of two iterations: the loop of learn() written out by hand on a net built WITHOUT the knobs -- per step the four rates of
    loss_options_ref.annealed_rates32, per micro-batch the columns cut with torch indexing (old_values among them)."""
    from ddrl4nav_amd import ops
    from ddrl4nav_amd._lib import STATS_FLOATS, check
    from ddrl4nav_amd.ops import _p, _st
    x = X.cell_inputs(cell)
    n, N_STEPS, FLOOR, OPT = cell.n, 3, 0.25, (0.3, True)
    net = GX.make_net(cell, TRAINING_ITER_TIME=2, VALUE_CLIP=OPT[0], ENTROPY_BONUS_SPLIT=True, LR_ANNEAL_UPDATES=N_STEPS, CLIP_ANNEAL=True,
                      LR_ANNEAL_FLOOR=FLOOR)
    hand = GX.make_net(cell, TRAINING_ITER_TIME=2)
    assert net.loss_options == OPT and net.lr_anneal == (N_STEPS, FLOOR, True) and hand.lr_anneal is None
    items = []
    for _ in range(2):
        items += _run(net, _exp(cell, rows=[x.rets, x.old_values]))
    assert [ut for _, ut, _ in items] == [1, 2, 3, 4] and net.anneal_step == 4
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = [dev(s) for s in x.states]
    acts, old, adv, ret, vold = (dev(a) for a in (x.actions, x.old_logps, x.advs, x.rets, x.old_values))
    base = hand._base_rates
    rates = [LR.annealed_rates32(base, u, N_STEPS, FLOOR, True) for u in range(4)]
    assert rates[0] == [float(np.float32(b)) for b in base] and rates[3][0] == float(np.float32(base[0] * FLOOR)) and rates[3][3] < rates[0][3]     # u = 3: the floor holds
    for u in range(4):
        c = hand._cfg
        c.actor_lr, c.critic_lr, c.learning_rate, c.ppo_clip = rates[u]
        hand._ensure_packed()
        for ci, (lo, hi) in enumerate(X.chunks(cell)):
            sel = torch.arange(lo, hi, device="cuda")
            ha, hc = hand._features([s[sel].contiguous() for s in st], hi - lo)
            ops.heads_loss_opt(hand._hd, c, hand.params, ha, hc, hi - lo, acts[sel].contiguous(), old[sel].contiguous(), adv[sel].contiguous(),
                               ret[sel].contiguous(), OPT, vold[sel].contiguous(), n, hand._dh[0], hand._dh[1], hand.gtmp, hand._heads_ws)
            hand._backward_both(hand._dh[0], hand._dh[1], hi - lo)
            if ci == 0:
                hand.grads.copy_(hand.gtmp)
            else:
                check(hand.lib.ddrl_op_accumulate(_p(hand.grads), _p(hand.gtmp), hand.n_params + STATS_FLOATS, _st()))
        hand._step += 1
        check(hand.lib.ddrl_op_clip_adam(byref(c), _p(hand.params), _p(hand.grads), _p(hand.adam_m), _p(hand.adam_v), hand.n_params,
                                         hand.n_actor, 0, hand._step, _p(hand._adam_ws), _st()))
        hand._dirty = True
        s = hand.stats()
        assert all(items[u][0][k] == s[k] for k in LOSS_KEYS), (u, items[u][0], s)
        assert _same(items[u][2], _state(hand)), u
    # the schedule is seen: an un-annealed net leaves the first step alike and the later ones not
    plain = GX.make_net(cell, TRAINING_ITER_TIME=2, VALUE_CLIP=OPT[0], ENTROPY_BONUS_SPLIT=True)
    first = _run(plain, _exp(cell, rows=[x.rets, x.old_values]))
    assert _same(first[0][2], items[0][2]) and not torch.equal(first[1][2][0], items[1][2][0])


def test_an_extra_critic_on_a_shared_mlp_net_adds_its_loss_and_its_encoder_gradient():
    """PPO.add_critic on a shared MLP net, n = 67 in micro-batches of 32, 32 and 3: VLoss is the sum of both heads' value losses, the
    encoder's gradient carries both, and the extra head itself is no parameter of the net -- the step leaves it alone.  Against the
    float64 oracle with a second value head, tolerances of tests/test_generic_cross_gpu.py."""
    from ddrl4nav_amd.nn import Critic
    from ddrl4nav_amd.utils.recipe import hash_weights
    from oracle import ddrl_oracle_nav as N
    import heads_ref as H
    cell = X.Cell("mlp_shared", "cat5", 0, "default", "none", 0, 67, 32)
    x = X.cell_inputs(cell)
    n = cell.n
    rng = np.random.default_rng(X.cell_seed(cell))
    w2 = hash_weights([("critic_linear.weight", (1, 512)), ("critic_linear.bias", (1,))], X.cell_seed(cell) + 1)
    net = GX.make_net(cell)
    extra = Critic(device="cpu", last_input_dim=512)
    extra.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w2.items()})
    net.add_critic(extra)
    before = {k: p.detach().cpu().clone() for k, p in extra.named_parameters()}
    # float64: the oracle net and the second head on the same features
    W2, B2 = torch.from_numpy(w2["critic_linear.weight"]).double(), torch.from_numpy(w2["critic_linear.bias"]).double()
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    with torch.no_grad():
        v2_64 = (X.oracle_net(cell, x.weights).features([t(s) for s in x.states])[1] @ W2.T + B2)[:, 0].numpy()
    rets2 = (v2_64 + rng.normal(0, 1, n)).astype(np.float32)
    # forward: both values
    (_, logp), values = net(x.states, torch.from_numpy(x.actions))
    assert len(values) == 2
    np.testing.assert_allclose(values[0].cpu().numpy()[:, 0], x.v64, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(values[1].cpu().numpy()[:, 0], v2_64, rtol=2e-5, atol=2e-6)
    sub = GX.kernel_decisions(net, cell, x)
    onet = X.oracle_net(cell, x.weights)
    onet.prenet.sub = sub[0]
    total, al, vl, ent = N.losses(onet, [t(s) for s in x.states], t(x.actions), t(x.old_logps), t(x.advs), t(x.rets))
    v2 = (onet.features([t(s) for s in x.states])[1] @ W2.T + B2)[:, 0]
    vl2 = torch.mean((t(rets2) - v2) ** 2) / 2
    (total + vl2 * N.V_LOSS_THETA).backward()
    g64 = {k: p.grad.numpy() for k, p in onet.named_parameters()}
    norm, coef = H.clip_coef64(torch.cat([torch.from_numpy(g).reshape(-1) for g in g64.values()]), X.CLIP_GRAD_NUM, True)
    # the same without the second head: its share of the encoder gradient is not rounding noise
    lone = X.oracle_net(cell, x.weights)
    lone.prenet.sub = sub[0]
    N.losses(lone, [t(s) for s in x.states], t(x.actions), t(x.old_logps), t(x.advs), t(x.rets))[0].backward()
    enc = "prenet.fc0.0.weight"
    assert np.abs(lone.prenet.fc0[0].weight.grad.numpy() - g64[enc]).max() > 1e-2 * np.abs(g64[enc]).max()
    net.training_iter_time = 1
    items = _run(net, _exp(cell, rows=[x.rets, rets2]))
    assert len(items) == 1
    got = items[0][0]
    want = [(total + vl2 * N.V_LOSS_THETA).item(), al.item(), (vl + vl2).item(), ent.item()]
    print("extra critic losses: kernel %s, float64 %s (second head's value loss %.6g)" % ([got[k] for k in LOSS_KEYS], want, vl2.item()))
    np.testing.assert_allclose([got[k] for k in LOSS_KEYS], want, rtol=2e-5, atol=2e-6)
    stats = net.stats()
    np.testing.assert_allclose([stats["GradNorm"], stats["ClipCoef"]], [norm, coef], rtol=2e-5)
    flat, off = net.grads[:net.n_params].cpu().double().numpy(), 0
    for name, p in net.named_parameters():
        k = p.numel()
        wantg = g64[name].reshape(-1) * coef
        err, scale = np.abs(flat[off:off + k] - wantg).max(), np.abs(wantg).max()
        off += k
        print("extra critic %s: %.2e max|want|" % (name, err / scale))
        assert err <= 2e-5 * scale, (name, err / scale)
    for k, p in extra.named_parameters():
        assert torch.equal(p.detach().cpu(), before[k]), k
    assert not torch.equal(net.params.cpu(), torch.cat([torch.from_numpy(v).reshape(-1) for v in x.weights.values()]))
