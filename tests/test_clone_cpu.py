"""Host side of cloning a GenericPPO actor (ddrl4nav_amd/nn/dagger.py, data/demo_pool.py, runner/dagger_loop.py):
the float64 statement of a clone step and its fp32 form against half the GPU bound, the pool's cursor and wrap arithmetic, the mixing
schedule, the argument checks, the operators' refusals before HIP, and the refusals imitation_learning keeps."""
import ctypes

import numpy as np
import pytest
import torch

import clone_ref as C
import generic_cross as X


# ---- the statement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", C.CELLS, ids=C.cell_id)
def test_fp32_statement_lies_inside_half_the_gpu_bound(cell):
    """The bound the kernels are held to (tests/test_clone_gpu.py) is checked on the reference's own arithmetic first: the statement
    restated in fp32, under the same ReLU / max-pool decisions, is within half of it."""
    x, y = X.cell_inputs(cell), C.labels_of(cell)
    sub = C.fp32_decisions(cell, x, y)
    u64, u32 = C.clone_statement(cell, x, y, torch.float64, sub=sub), C.clone_statement(cell, x, y, torch.float32, sub=sub)
    assert abs(u32.loss - u64.loss) <= 0.5 * C.LOSS_RTOL * abs(u64.loss), (u32.loss, u64.loss)
    if X.gaussian(cell):
        assert abs(u32.metric - u64.metric) <= 0.5 * C.LOSS_RTOL * abs(u64.metric)
    side, worst = C.actor_side(cell), (0.0, "")
    for name, g64 in u64.grads.items():
        if not name.startswith(side):
            assert g64 is None, name                                  # the critic side and log_std take no part
            continue
        assert g64 is not None and g64.any(), name
        err, scale = np.abs(u32.grads[name] - g64).max(), np.abs(g64).max()
        worst = max(worst, (err / scale, name))
        assert err <= 0.5 * C.GRAD_BOUND * scale, (name, err / scale)
    print("%s: loss %.9g, fp32 statement's worst tensor %s at %.2e max|want|" % (C.cell_id(cell), u64.loss, worst[1], worst[0]))


def test_statement_is_the_loss_it_names():
    cell = C.CELLS[0]
    x, y = X.cell_inputs(cell), C.labels_of(cell)
    u = C.clone_statement(cell, x, y)
    assert y.shape == (37, 3) and u.mu.shape == (37, 3)
    assert u.loss == pytest.approx(((u.mu - y) ** 2).sum() / (2 * 37 * 3), rel=1e-12)
    assert u.metric == pytest.approx(np.abs(u.mu - y).sum(), rel=1e-12)
    assert u.grads["actor.log_std"] is None and u.grads["critic.critic_linear.weight"] is None
    cat = C.CELLS[1]
    yc = C.labels_of(cat)
    assert yc.shape == (37, 1) and set(np.unique(yc)) <= set(range(5))
    uc = C.clone_statement(cat, X.cell_inputs(cat), yc)
    lse = np.log(np.exp(uc.mu).sum(1))
    assert uc.loss == pytest.approx(float((lse - uc.mu[np.arange(37), yc[:, 0].astype(int)]).mean()), rel=1e-12)


# ---- DemoPool -----------------------------------------------------------------------------------------------------------------------------
def test_pool_cursor_and_wrap_arithmetic():
    from ddrl4nav_amd.data import demo_pool as D
    assert [D.slot_of(t, 3) for t in range(7)] == [0, 1, 2, 0, 1, 2, 0]
    rows = lambda *a: D.labelled_rows(*a).tolist()
    assert rows(0, False, 3, 2) == [] and rows(1, True, 3, 2) == []
    assert rows(1, False, 3, 2) == [0, 1] and rows(2, True, 3, 2) == [0, 1]
    assert rows(3, True, 3, 2) == [0, 1, 2, 3] and rows(3, False, 3, 2) == [0, 1, 2, 3, 4, 5]
    assert rows(4, True, 3, 2) == [2, 3, 4, 5]                       # the waiting set has overwritten slot 0
    assert rows(4, False, 3, 2) == [0, 1, 2, 3, 4, 5] and rows(9, True, 3, 2) == [0, 1, 2, 3]
    assert D.labelled_rows(5, True, 4, 3).dtype == np.int64


def test_pool_argument_checks():
    from ddrl4nav_amd.data import DemoPool
    for args, kw in ((([(5,)], 2, 7), dict(n_envs=2)), (([(5,)], 2, 2), dict(n_envs=2)), (([(5,)], 0, 8), dict(n_envs=2)),
                     (([(5,)], 2, 8), dict(n_envs=0)), (([], 2, 8), dict(n_envs=2)), (([(5, 0)], 2, 8), dict(n_envs=2))):
        with pytest.raises(ValueError):
            DemoPool(*args, device="cpu", **kw)
    pool = DemoPool([(1, 4), (5,)], 2, 6, device="cpu", n_envs=2)       # the bookkeeping needs no GPU
    assert [tuple(c.shape) for c in pool.components] == [(6, 1, 4), (6, 5)] and tuple(pool.labels.shape) == (6, 2) and len(pool) == 0
    comps, lab = pool.rows(4)                                           # set 4 lives in slot 1: views, not copies
    assert comps[1].data_ptr() == pool.components[1][2:].data_ptr() and lab.data_ptr() == pool.labels[2:].data_ptr()
    assert pool.open() == 0 and pool.pending and len(pool) == 0
    with pytest.raises(RuntimeError):
        pool.open()
    pool.close_label()
    with pytest.raises(RuntimeError):
        pool.close_label()
    assert len(pool) == 2
    pool.put([np.ones((4, 1, 4)), np.ones((4, 5))], np.full((4, 2), 0.5))
    assert pool.cursor == 3 and len(pool) == 6 and float(pool.labels[:2].sum()) == 0.0 and float(pool.labels[2:].sum()) == 4.0
    with pytest.raises(ValueError):
        pool.put([np.ones((3, 1, 4)), np.ones((3, 5))], np.ones((3, 2)))
    assert pool.open() == 3 and pool.labelled_rows().tolist() == [2, 3, 4, 5]


# ---- the loop's host side -------------------------------------------------------------------------------------------------------------------
def test_default_betas_and_loop_checks():
    from ddrl4nav_amd.runner import dagger_loop as L
    assert L.default_betas(1) == [1.0] and L.default_betas(2) == [1.0, 0.0] and L.default_betas(5) == [1.0, 0.75, 0.5, 0.25, 0.0]
    with pytest.raises(ValueError):
        L.default_betas(0)

    class Stub:
        pass

    env, other, expert, pool, net = Stub(), Stub(), Stub(), Stub(), Stub()
    env.N, env.state_shapes, env.device = 4, [(1, 960), (5,), (3, 48, 48)], torch.device("cpu")
    expert.env = env
    pool.n_envs, pool.action_dim, pool.device = 4, 2, torch.device("cpu")
    pool.components = [torch.zeros((8,) + s) for s in env.state_shapes]
    net.continuous, net.n_actions = True, 2
    L._check(net, env, expert, pool)
    for obj, name, value in ((expert, "env", other), (pool, "n_envs", 8), (pool, "action_dim", 3), (net, "continuous", False),
                             (net, "n_actions", 3), (pool, "components", pool.components[:2]), (pool, "device", torch.device("meta"))):
        keep = getattr(obj, name)
        setattr(obj, name, value)
        with pytest.raises(ValueError):
            L._check(net, env, expert, pool)
        setattr(obj, name, keep)
    with pytest.raises(ValueError):
        L.collect(net, env, expert, pool, 0, 1.0)
    with pytest.raises(ValueError):
        list(L.run(net, env, expert, pool, 3, 4, betas=[1.0, 0.5]))


def test_clone_trainer_argument_checks():
    from ddrl4nav_amd.nn import dagger as G
    with pytest.raises(TypeError, match="GenericPPO"):
        G.CloneTrainer(object(), None, 1e-3)
    order = G.epoch_order(np.arange(10, 30), 5, 0)
    assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(10, 30))
    assert np.array_equal(order, G.epoch_order(np.arange(10, 30), 5, 0)) and not np.array_equal(order, G.epoch_order(np.arange(10, 30), 5, 1))
    assert not np.array_equal(order, G.epoch_order(np.arange(10, 30), 6, 0))
    from ddrl4nav_amd.nn.generic import GenericPPO
    assert callable(GenericPPO.clone_actor)


def test_imitation_learning_keeps_its_refusals():
    from ddrl4nav_amd.nn.imitation import check_supported

    class Gaussian:
        class actor:
            log_std = 0

    with pytest.raises(NotImplementedError, match="regression"):
        check_supported(object(), "regression")
    with pytest.raises(NotImplementedError, match="Categorical actor"):
        check_supported(Gaussian(), "classification")
    with pytest.raises(NotImplementedError, match="Atari PPO net only"):
        check_supported(object(), "classification")
    with pytest.raises(ValueError):
        check_supported(object(), "ranking")


# ---- the operators' refusals, decided before HIP ------------------------------------------------------------------------------------------
def test_bc_mse_refusals():
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    f = ctypes.c_int64()
    assert lib.ddrl_op_heads_bc_mse_ws_floats(0, 8, f) == -2 and lib.ddrl_op_heads_bc_mse_ws_floats(9, 8, f) == -2
    assert lib.ddrl_op_heads_bc_mse_ws_floats(2, 0, f) == -1 and lib.ddrl_op_heads_bc_mse_ws_floats(2, 8, None) == -1
    a, M = 0x10000000, 0x100000
    ok = dict(w=a, b=a + M, A=2, h=a + 2 * M, ld_h=512, n=4, y=a + 3 * M, n_total=4, dh=a + 4 * M, ld_dh=512, dw=a + 5 * M, db=a + 6 * M,
              stats=a + 7 * M, ws=a + 8 * M)
    for bad, code in ((dict(A=0), -2), (dict(A=9), -2), (dict(n=0), -1), (dict(n_total=3), -1), (dict(ld_h=508), -1), (dict(ld_dh=514), -1),
                      (dict(h=a + 2 * M + 4), -1), (dict(dh=a + 4 * M + 8), -1), (dict(y=None), -1), (dict(stats=None), -1),
                      (dict(y=a + 3 * M + 2), -1)):
        kw = dict(ok, **bad)
        assert lib.ddrl_op_heads_bc_mse(*[kw[k] for k in ok], None) == code, bad


def test_gather_rows_f32_refusals():
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    a, M = 0x10000000, 0x1000000
    ok = dict(src=a, n_rows=10, row=5, idx=a + M, n=4, dst=a + 2 * M)
    for bad in (dict(src=None), dict(idx=None), dict(dst=None), dict(n=0), dict(n_rows=0), dict(row=0), dict(src=a + 2), dict(dst=a + 2 * M + 1),
                dict(idx=a + M + 2), dict(dst=a + 196), dict(dst=a + M + 12), dict(dst=a - 76), dict(row=2 ** 62)):
        kw = dict(ok, **bad)
        assert lib.ddrl_op_gather_rows_f32(*[kw[k] for k in ok], None) == -1, bad
