"""The claims of tests/generic_cross.py, the extended float64 statement (oracle/ddrl_oracle_nav.py: losses / learn with the knobs) at its
defaults, and the yardstick of tests/test_generic_cross_gpu.py on its own: in every cell the fp32 oracle, running under its own ReLU /
max-pool decisions, sits within HALF the bounds the GPU test applies to the kernels -- 1e-5 max|g64| per tensor of 2e-5, half the forward
and loss tolerances -- from the float64 oracle under the same decisions.  A cell where the fp32 reference itself used up the bound could
not tell a kernel fault from summation noise; such a cell gets other inputs (generic_cross.SALT), never a wider bound."""
import time

import numpy as np
import pytest
import torch

import generic_cross as X
import heads_ref as H
from oracle import ddrl_oracle_nav as N
from oracle.ddrl_oracle import (CLIP_GRAD_NUM, DUEL_PPO_CLIP, ENT_LOSS_THETA, PPO_CLIP, V_LOSS_THETA)


def test_cells_are_a_pairwise_covering_array():
    assert X.uncovered_pairs() == []
    assert 20 <= len(X.CELLS) <= 24 and len(set(X.CELLS)) == len(X.CELLS)
    # the table helper must be able to fail: without its only (nav1d_split, gauss3) cell that pair is reported
    rest = [c for c in X.CELLS if (c.net, c.head) != ("nav1d_split", "gauss3")]
    assert ("net", "nav1d_split", "head", "gauss3") in X.uncovered_pairs(rest)


def test_ids_and_seeds_are_unique_and_every_cell_can_be_built():
    ids, seeds = [X.cell_id(c) for c in X.CELLS], [X.cell_seed(c) for c in X.CELLS]
    assert len(set(ids)) == len(ids) and len(set(seeds)) == len(seeds)
    for c in X.CELLS:
        assert X.is_buildable(c), c
        assert (c.n, c.max_batch) in X.BATCHES and c.smooth_l1 in X.SMOOTH_L1 and c.diag in X.DIAG
        assert sum(hi - lo for lo, hi in X.chunks(c)) == c.n and all(hi - lo <= c.max_batch for lo, hi in X.chunks(c))
    assert [hi - lo for lo, hi in X.chunks(X.Cell("mlp_split", "cat5", 0, "default", "none", 0, 7, 3))] == [3, 3, 1]
    assert [hi - lo for lo, hi in X.chunks(X.Cell("mlp_split", "cat5", 0, "default", "none", 0, 150, 131))] == [131, 19]
    # the places the issue names: a Gaussian head over a shared encoder, a categorical one over NavPreNet1D x2, a shared MLP
    assert any(X.shared(c) and X.gaussian(c) for c in X.CELLS)
    assert any(c.net == "nav1d_split" and not X.gaussian(c) for c in X.CELLS)
    assert any(c.net == "mlp_shared" for c in X.CELLS)
    assert any(not X.shared(c) and X.gaussian(c) and X.options(c)[1] for c in X.CELLS)      # the entropy gradient reaches log_std


# ---- the extended oracle at its defaults ---------------------------------------------------------------------------------------------------
def _losses_before(net, states, actions, old_logps, advs, rets):
    """oracle_nav.losses as it stood before it took keyword arguments, verbatim."""
    _, log_p, ent_el, v = net(states, actions)
    ratio = torch.exp(log_p - old_logps)
    m = torch.min(ratio * advs, torch.clamp(ratio, 1.0 - PPO_CLIP, 1.0 + PPO_CLIP) * advs)
    actor_loss = -torch.mean(torch.where(advs > 0, m, torch.max(m, DUEL_PPO_CLIP * advs)))
    v_loss = torch.mean((rets - v.squeeze()) ** 2) / 2
    ent = torch.mean(ent_el)
    return actor_loss + v_loss * V_LOSS_THETA - ent * ENT_LOSS_THETA, actor_loss, v_loss, ent


def _learn_before(net, optims, states, actions, old_logps, advs, rets):
    """One iteration of oracle_nav.learn as it stood, verbatim."""
    total, actor_loss, v_loss, ent = _losses_before(net, states, actions, old_logps, advs, rets)
    for o in optims:
        o.zero_grad()
    if net.shared:
        total.backward()
    else:
        actor_loss.backward()
        v_loss.backward()
    gnorm = torch.nn.utils.clip_grad_norm_(net.parameters(), CLIP_GRAD_NUM)
    for o in optims:
        o.step()
    return [total.item(), actor_loss.item(), v_loss.item(), ent.item(), float(gnorm)]


DEFAULT_CELLS = [X.Cell("mlp_split", "cat5", 0, "default", "none", 0, 37, 37), X.Cell("mlp_shared", "gauss3", 0, "default", "none", 0, 37, 37),
                 X.Cell("mlp_split", "gauss1", 0, "default", "none", 0, 7, 3), X.Cell("navpre_shared", "cat9", 0, "default", "none", 0, 7, 3)]


@pytest.mark.parametrize("cell", DEFAULT_CELLS, ids=X.cell_id)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_extended_oracle_equals_the_old_one_bit_for_bit_at_the_defaults(cell, dtype):
    x = X.cell_inputs(cell)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    args = ([t(s) for s in x.states], t(x.actions), t(x.old_logps), t(x.advs), t(x.rets))
    new, old = X.oracle_net(cell, x.weights, dtype), X.oracle_net(cell, x.weights, dtype)
    for a, b in zip(N.losses(new, *args), _losses_before(old, *args)):
        assert torch.equal(a, b)
    # spelled-out defaults are the defaults
    for a, b in zip(N.losses(new, *args, hyper=dict(H.DEFAULT_HYPER), smooth_l1=False, value_clip=0.0, old_values=None),
                    _losses_before(old, *args)):
        assert torch.equal(a, b)
    ld = next(N.learn(new, new.make_optims(), *args, iters=1))[0]
    want = _learn_before(old, old.make_optims(), *args)
    assert [ld[k] for k in ("PpoTotalLoss", "ActorLoss", "VLoss", "EntLoss", "GradNorm")] == want
    for (k, p), (_, q) in zip(new.named_parameters(), old.named_parameters()):
        assert torch.equal(p, q) and torch.equal(p.grad, q.grad), k


def test_the_knobs_mean_what_loss_options_ref_states():
    """oracle_nav.losses / backward with every knob against tests/loss_options_ref.py:loss_block on the same 512-wide features: an oracle
    net whose encoders are replaced by the case's features (both families, both sharing modes)."""
    import loss_options_ref as LR
    for cont, A, shared, smooth, name in ((0, 5, 0, 1, "both"), (1, 3, 1, 0, "clip"), (1, 2, 0, 1, "entropy"), (0, 9, 1, 0, "both")):
        c = LR.make_case(cont, A, 67, shared, smooth, LR.OPTION_SETS[name], hyper=H.OTHER_HYPER, seed=5)
        want = LR.loss_block(c, torch.float64)
        net = N.OracleNet(lambda: N.MLPPreNet(4, 512), A, bool(cont), bool(shared)).double()
        with torch.no_grad():
            net.actor.actor_linear.weight.copy_(c.params["actor_w"])
            net.actor.actor_linear.bias.copy_(c.params["actor_b"])
            net.critic.critic_linear.weight.copy_(c.params["critic_w"][None])
            net.critic.critic_linear.bias.copy_(c.params["critic_b"])
            if cont:
                net.actor.log_std.copy_(c.params["log_std"])
        ha = c.ha.double()
        net.features = lambda states, ha=ha, hc=(ha if shared else c.hc.double()): (ha, hc)
        parts = N.losses(net, None, c.actions.double(), c.old_logps.double(), c.advs.double(), c.rets.double(), hyper=c.hyper,
                         smooth_l1=bool(smooth), value_clip=c.value_clip, old_values=c.old_values.double())
        N.backward(net, *parts, hyper=c.hyper, entropy_split=c.entropy_split)
        # loss_block reports the Gaussian entropy per sample (mean over D first): the same mean
        np.testing.assert_allclose([p.item() for p in parts[1:]], want["losses"].numpy(), rtol=1e-12, atol=1e-14)
        pairs = [(net.actor.actor_linear.weight, "g_actor_w"), (net.actor.actor_linear.bias, "g_actor_b"),
                 (net.critic.critic_linear.bias, "g_critic_b")] + ([(net.actor.log_std, "g_log_std")] if cont else [])
        for p, key in pairs:
            np.testing.assert_allclose(p.grad.numpy(), want[key].numpy(), rtol=1e-10, atol=1e-15, err_msg=key)
        np.testing.assert_allclose(net.critic.critic_linear.weight.grad.numpy()[0], want["g_critic_w"].numpy(), rtol=1e-10, atol=1e-15)


# ---- the recipe and the room it leaves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", X.CELLS, ids=X.cell_id)
def test_recipe_keeps_its_promises_and_the_fp32_oracle_is_inside_half_the_gpu_bounds(cell):
    t0 = time.time()
    x = X.cell_inputs(cell)
    assert x is X.cell_inputs(cell)                       # computed once, shared
    n = cell.n
    assert all(s.shape[0] == n and s.dtype == np.float32 for s in x.states)
    assert all(a.shape == (n,) and a.dtype == np.float32 for a in (x.old_logps, x.advs, x.rets, x.old_values))
    assert x.actions.shape == ((n, X.n_out(cell)) if X.gaussian(cell) else (n,))
    if not X.gaussian(cell):
        assert x.actions.min() >= 0 and x.actions.max() <= X.n_out(cell) - 1 and np.array_equal(x.actions, np.floor(x.actions))
    X.check_recipe(cell, x)
    # the fp32 oracle under its own decisions, the float64 oracle under the same ones
    n_enc = 1 if X.shared(cell) else 2
    record = [{} for _ in range(n_enc)]
    u32 = X.oracle_update(cell, x, torch.float32, record=record)
    u64 = X.oracle_update(cell, x, torch.float64, sub=[X.relu_of(r) for r in record])
    worst = (0.0, "")
    assert list(u32.grads) == list(u64.grads)
    for name, g64 in u64.grads.items():
        g32 = u32.grads[name]
        if g64 is None:
            assert g32 is None, name
            continue
        scale = np.abs(g64).max()
        if scale == 0.0:
            assert not g32.any(), name
            continue
        err = np.abs(g32 - g64).max() / scale
        worst = max(worst, (err, name))
        assert err <= 1e-5, (name, err)
    np.testing.assert_allclose(u32.losses, u64.losses, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(u32.norm, u64.norm, rtol=1e-5)
    # forward: half of value rtol 2e-5 / atol 2e-6, logp rtol 2e-5 / atol 2e-5, entropy rtol 1e-5 / atol 1e-6, probs or mu rtol 2e-5 / atol 2e-6
    with torch.no_grad():
        t = lambda a: torch.from_numpy(np.asarray(a))
        d32, l32, e32, v32 = X.oracle_net(cell, x.weights, torch.float32)([t(s) for s in x.states], t(x.actions))
    d64, l64, e64, v64 = x.dist64, x.logp64, x.ent64, x.v64
    np.testing.assert_allclose(v32.numpy()[:, 0], v64, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(l32.numpy(), l64, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(e32.numpy(), e64, rtol=5e-6, atol=5e-7)
    np.testing.assert_allclose(d32.numpy(), d64, rtol=1e-5, atol=1e-6)
    print("%s: fp32 oracle against float64, worst tensor %s: %.2e max|g64| (%.1f s)" % (X.cell_id(cell), worst[1], worst[0], time.time() - t0))
