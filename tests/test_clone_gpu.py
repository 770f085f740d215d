"""One clone step of GenericPPO (ddrl4nav_amd/nn/dagger.py CloneTrainer) against its float64 statement
(tests/clone_ref.py) on five cells of tests/generic_cross.py: both head families, split and shared encoders, NavPreNet1D x2, and a batch
above max_batch folded from micro-batches.

Stated tolerances: loss and metric rtol 2e-5; actor-side gradients per tensor |d| <= 2e-5 max|want| (tests/test_generic_cross_gpu.py),
want = the float64 gradient under the kernels' ReLU / max-pool decisions; the optimiser step by the element-wise criterion of
test_heads_optim_ops_gpu.test_clip_adam_one_step_element_by_element.  Everything outside the actor side is held to bit equality."""
import numpy as np
import pytest
import torch

import clone_ref as C
import generic_cross as X
import heads_ref as H

pytestmark = pytest.mark.gpu


def filled_pool(cell, x, net):
    from ddrl4nav_amd.data import DemoPool
    y = C.labels_of(cell)
    pool = DemoPool([s.shape[1:] for s in x.states], y.shape[1], cell.n + 3, device=net.device)
    pool.put(x.states, y)
    assert pool.labelled_rows().tolist() == list(range(cell.n))
    return pool, y


@pytest.mark.parametrize("cell", C.CELLS, ids=C.cell_id)
def test_clone_step_vs_float64(cell):
    import test_generic_cross_gpu as GX
    from test_heads_optim_ops_gpu import F32, _elementwise, _torch_adam32
    from ddrl4nav_amd.nn.dagger import CloneTrainer
    tag = C.cell_id(cell)
    x, n = X.cell_inputs(cell), cell.n
    net = GX.make_net(cell)
    pool, y = filled_pool(cell, x, net)
    side = C.actor_side(cell)
    names = [k for k, _ in net.named_parameters()]
    # ---- the decisions the step will take, then the float64 statement under them
    sub = GX.kernel_decisions(net, cell, x)[0]
    u64, u32 = C.clone_statement(cell, x, y, torch.float64, sub=sub), C.clone_statement(cell, x, y, torch.float32, sub=sub)
    (before, _), _ = net(x.states, None, True)
    before = before.clone()
    # ---- one step
    p0 = net.params.clone()
    trainer = CloneTrainer(net, pool, C.LR)
    row = torch.zeros(2).pin_memory()
    idx = torch.arange(n, dtype=torch.int32, device=net.device)
    trainer.step(idx, n, row)
    torch.cuda.synchronize()
    assert trainer.step_count == 1 and net._step == 0 and net.update_time == 0
    print("%s: loss %.9g (float64 %.9g), metric %.9g (%.9g)" % (tag, float(row[0]), u64.loss, float(row[1]), u64.metric))
    np.testing.assert_allclose(float(row[0]), u64.loss, rtol=C.LOSS_RTOL, err_msg=tag)
    if X.gaussian(cell):
        np.testing.assert_allclose(float(row[1]), u64.metric, rtol=C.LOSS_RTOL, err_msg=tag)
    else:
        assert float(row[1]) == u64.metric, tag
    # ---- gradients: the actor side against float64, everything else exactly zero
    flat = net.grads[:net.n_params].cpu()
    assert bool(torch.isfinite(net.grads).all()) and bool(torch.isfinite(net.params).all())
    off, failed, worst = 0, [], (0.0, 0.0, "")
    for name, p in net.named_parameters():
        k = p.numel()
        g = flat[off:off + k].double().numpy().reshape(tuple(p.shape))
        off += k
        if not name.startswith(side):
            assert u64.grads[name] is None and not g.any(), (tag, name, "outside the actor side the gradient is exactly zero")
            continue
        want = u64.grads[name]
        scale, err = np.abs(want).max(), np.abs(g - want).max()
        err32 = np.abs(u32.grads[name] - want).max()
        worst = max(worst, (err / scale, err / max(err32, 2.0 ** -24 * scale), name))
        if not err <= C.GRAD_BOUND * scale:
            failed.append((name, err / scale))
    print("%s gradient vs float64, worst tensor %s: %.2e max|want|, %.2f x the fp32 statement's error" % (tag, worst[2], worst[0], worst[1]))
    assert off == net.n_params and not failed, (tag, failed)
    # ---- the step: one Adam group at lr over the whole arena, no clipping, on the kernel's own gradient
    c = trainer._opt_cfg
    lr, b1, b2, eps = F32(c.learning_rate), F32(c.adam_beta1), F32(c.adam_beta2), F32(c.adam_eps)
    assert lr == F32(C.LR) and c.clip_grad == 0
    parts = [(0, net.n_params, lr)]
    p0c = p0.cpu()
    zeros = torch.zeros_like(p0c)
    lr64 = torch.full((net.n_params,), lr, dtype=torch.float64)
    upd64, m64, v64, g64 = H.adam64(p0c.double(), flat.double(), zeros.double(), zeros.double(), lr64, 1, b1, b2, eps, 1.0)
    p32, m32, v32 = _torch_adam32(p0c, flat, zeros, zeros, parts, 1, (b1, b2), eps, False, 0.0)
    pk, mk, vk = net.params.cpu().double(), trainer.m.cpu().double(), trainer.v.cpu().double()
    tiny = torch.tensor(2.0 ** -126, dtype=torch.float64)
    floor = lambda s: torch.where(s == 0, s, torch.maximum(s, tiny))
    _elementwise("clone_adam_m", mk, m64, m32, floor(g64.abs()), net.n_params, tag)
    _elementwise("clone_adam_v", vk, v64, v32, floor(v64), net.n_params, tag)
    step_lr = lr64 / (1.0 - b1)
    zero_p = p0c == 0
    for sel, key in ((zero_p, "clone_adam_update"), (~zero_p, "clone_adam_update_rounded_into_p")):
        if bool(sel.any()):
            _elementwise(key, (pk - p0c.double())[sel], upd64[sel], (p32 - p0c.double())[sel],
                         torch.maximum(torch.maximum(step_lr, upd64.abs()), p0c.double().abs())[sel], net.n_params, tag)
    # ---- the critic side, log_std and the PPO optimiser's state: bit-unchanged
    moved = 0
    for name, p in net.named_parameters():
        o = net._offsets[name]
        same = torch.equal(net.params[o:o + p.numel()].view(torch.int32), p0[o:o + p.numel()].view(torch.int32))
        if name.startswith(side):
            moved += 0 if same else 1
        else:
            assert same, (tag, name, "moved by a clone step")
    assert moved == sum(1 for k in names if k.startswith(side)), (tag, "an actor-side tensor did not move")
    assert not bool(net.adam_m.any()) and not bool(net.adam_v.any()) and net._step == 0
    # ---- forward afterwards runs on the new weights: the float64 oracle loaded with them
    (after, _), _ = net(x.states, None, True)
    new_w = {k: net.params[net._offsets[k]:net._offsets[k] + v.size].cpu().numpy().reshape(v.shape) for k, v in x.weights.items()}
    want = X.forward64(cell, new_w, x.states, np.zeros((n, X.n_out(cell))) if X.gaussian(cell) else np.zeros(n))[0]
    np.testing.assert_allclose(after.cpu().numpy(), want, rtol=2e-5, atol=2e-6, err_msg=tag)
    assert not torch.equal(after, before)


@pytest.mark.parametrize("cell", [C.CELLS[0], C.CELLS[1]], ids=C.cell_id)
def test_learn_after_cloning_is_learn_on_a_fresh_net(cell):
    """A clone step leaves nothing behind but the weights: net.learn afterwards equals learn on a fresh net loaded with the same
    state_dict, bit for bit."""
    import test_generic_cross_gpu as GX
    x = X.cell_inputs(cell)
    net = GX.make_net(cell)
    pool, _ = filled_pool(cell, x, net)
    log = net.clone_actor(pool, C.LR, 16, 2, seed=4)
    assert [r[:2] for r in log] == [(e, k) for e in (1, 2) for k in range(3)] and net.clone_log is log
    fresh = GX.make_net(cell)
    fresh.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    assert torch.equal(fresh.params, net.params)
    small = X.Cell(*cell[:6], 7, cell.max_batch)
    xs = X.Inputs(x.weights, [s[:7] for s in x.states], *[a[:7] for a in x[2:7]], *x[7:])
    for m in (net, fresh):
        items = list(m.learn(GX.experience(small, xs)))
        assert len(items) == 1
    assert torch.equal(fresh.params.view(torch.int32), net.params.view(torch.int32))
    assert torch.equal(fresh.adam_m, net.adam_m) and torch.equal(fresh.adam_v, net.adam_v) and fresh._step == net._step == 1
    assert torch.equal(fresh.grads.view(torch.int32), net.grads.view(torch.int32))


def test_clone_trainer_refusals():
    import test_generic_cross_gpu as GX
    from ddrl4nav_amd.data import DemoPool
    from ddrl4nav_amd.nn.dagger import CloneTrainer
    cell = C.CELLS[0]
    net = GX.make_net(cell)
    good = DemoPool([(4,)], 3, 8, device=net.device)
    for pool in (DemoPool([(4,), (5,)], 3, 8, device=net.device), DemoPool([(4,)], 2, 8, device=net.device)):
        with pytest.raises(ValueError):
            CloneTrainer(net, pool, 1e-3)
    for lr in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            CloneTrainer(net, good, lr)
    with pytest.raises(ValueError, match="no labelled row"):
        net.clone_actor(good, 1e-3, 4, 1, seed=0)
    net.gail_critic = True
    with pytest.raises(NotImplementedError, match="GAIL"):
        CloneTrainer(net, good, 1e-3)
