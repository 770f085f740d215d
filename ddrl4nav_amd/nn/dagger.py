"""Behaviour cloning of the actor side of a GenericPPO net from a demonstration pool on the device.

nn/imitation.py clones the Atari PPO net's Categorical actor and refuses everything else, as the reference's classification reader is
registered for atari only.  CloneTrainer is its counterpart for the operator-composed nets: any encoder GenericPPO takes, both head
families, SHARE_CNN_NET on and off.  What is trained is the actor's encoder (``actor.pre`` or the shared ``prenet``) and ``actor_linear``:

  * Gaussian actor: ``loss = mean((mu - y)^2) / 2`` over the batch's n * A elements, the regression loss the reference left commented
    (nn/base.py:142); ``log_std`` gets no gradient.  Categorical actor: ``F.cross_entropy(logits, y.long())``, as nn/imitation.py.
  * its own Adam (torch's defaults, one group at `lr`, no clipping) with private m / v / step: the PPO optimiser's state is never touched.

One step: ddrl_op_gather_rows_f32 per observation component and for the labels -> the actor encoder's forward_dev -> ddrl_op_heads_bc_mse
or ddrl_op_heads_bc_loss into d(h) and the ``actor_linear`` gradient views -> backward_dev -> ddrl_op_clip_adam.  The operators write
into the views bound to ``net.gtmp``; it is zeroed before the step and the optimiser runs over the whole arena: with a zero gradient
and zero private moments Adam's update is exactly 0, so the critic side and ``log_std`` stay bit-unchanged.  A batch above ``net.cap``
runs as micro-batches folded with ``fold_gradient``, as ``learn`` does.  No host synchronisation per step: (loss, metric) go to a pinned
row.
"""
from ctypes import byref

import numpy as np
import torch

from ddrl4nav_amd import _lib, ops
from ddrl4nav_amd._lib import check
from ddrl4nav_amd.data.demo_pool import same_device
from ddrl4nav_amd.ops import _p, _st

FEAT = 512


def check_clonable(net):
    """TypeError / NotImplementedError, naming the reason, for a net CloneTrainer does not take."""
    from ddrl4nav_amd.nn.generic import GenericPPO
    if not isinstance(net, GenericPPO):
        raise TypeError("CloneTrainer clones the actor of a GenericPPO net, got %s (the Atari PPO net has nn/imitation.py)"
                        % type(net).__name__)
    if net.gail_critic or net._extra:
        raise NotImplementedError("cloning a GAIL generator is not built: its extra critic shares the encoder the clone step trains")
    if net._raw_u8:
        raise NotImplementedError("cloning is built for fp32 observation components; a uint8 frame encoder has nn/imitation.py")
    if net.continuous and not 1 <= net.n_actions <= 8:
        raise NotImplementedError("the regression head takes 1..8 action dimensions, this actor has %d" % net.n_actions)
    if not net.continuous and not 2 <= net.n_actions <= 18:
        raise NotImplementedError("the classification head takes 2..18 actions, this actor has %d" % net.n_actions)


class CloneTrainer:
    """The device side of cloning `net`'s actor: staging rows for a micro-batch, the loss head's scratch, the private Adam state."""

    def __init__(self, net, pool, lr):
        check_clonable(net)
        lr = float(lr)
        if not (lr > 0.0 and np.isfinite(lr)):
            raise ValueError("lr must be positive and finite, got %r" % lr)
        enc = net._encs[0]
        if len(pool.components) != enc.n_inputs:
            raise ValueError("the pool holds %d observation components, the actor's encoder reads %d" % (len(pool.components), enc.n_inputs))
        want = net.n_actions if net.continuous else 1
        if pool.action_dim != want:
            raise ValueError("the pool's labels are %d wide, this actor's are %d" % (pool.action_dim, want))
        if not same_device(pool.device, net.device):
            raise ValueError("the pool lives on %s, the net on %s" % (pool.device, net.device))
        self.net, self.pool, self.lr = net, pool, lr
        f32 = dict(dtype=torch.float32, device=net.device)
        A, cap = net.n_actions, net.cap
        with torch.cuda.device(net.device):
            self.stage = [torch.empty((cap,) + tuple(c.shape[1:]), **f32) for c in pool.components]
            self.labels = torch.empty((cap, pool.action_dim), **f32)
            self.m, self.v = torch.zeros(net.n_params, **f32), torch.zeros(net.n_params, **f32)
            floats = ops.heads_bc_mse_ws_floats(A, cap) if net.continuous else ops.heads_bc_ws_floats(A, cap)
            self._ws = torch.empty(floats, **f32)
        self.step_count = 0
        # one group over the whole arena at `lr`, no clipping (the reference's Adam(self.parameters(), lr)); the private moments of
        # everything outside the actor side stay zero
        self._opt_cfg = _lib.default_config(max_batch=cap, share_cnn_net=1, clip_grad=0, learning_rate=lr)

    def set_lr(self, lr):
        lr = float(lr)
        if not (lr > 0.0 and np.isfinite(lr)):
            raise ValueError("lr must be positive and finite, got %r" % lr)
        self.lr = self._opt_cfg.learning_rate = lr

    def step(self, idx, n, stats_row=None):
        """One optimiser step on the n pool rows idx[:n] (int32 on the device); nothing waits for the host.  stats_row: a pinned [2]
        host row that receives (loss, metric) asynchronously -- metric: sum |mu - y| (Gaussian) or the correct count (Categorical)."""
        net, pool = self.net, self.pool
        o, A = net._offsets, net.n_actions
        w, b = net.params[o["actor.actor_linear.weight"]:], net.params[o["actor.actor_linear.bias"]:]
        lin = net.actor.actor_linear
        enc, dha = net._encs[0], net._dh[0]
        net._ensure_packed()
        net.gtmp.zero_()       # what no operator of the step writes -- the critic side, log_std -- is a zero gradient
        for lo, hi in net.chunks(n):
            k = hi - lo
            for src, dst in zip(pool.components, self.stage):
                ops.gather_rows_f32(src, idx[lo:hi], dst, k)
            ops.gather_rows_f32(pool.labels, idx[lo:hi], self.labels, k)
            ha = enc.forward_dev([s[:k] for s in self.stage], k)
            loss = ops.heads_bc_mse if net.continuous else ops.heads_bc_loss
            loss(w, b, A, ha, FEAT, k, self.labels, n, dha, FEAT, lin.weight.grad_view, lin.bias.grad_view, net.gtmp[net.n_params:],
                 self._ws)
            enc.backward_dev(dha, k)
            net.fold_gradient(lo == 0)
        self.step_count += 1
        check(net.lib.ddrl_op_clip_adam(byref(self._opt_cfg), _p(net.params), _p(net.grads), _p(self.m), _p(self.v), net.n_params,
                                        net.n_params, 1, self.step_count, _p(net._adam_ws), _st()))
        net.params_changed()
        if stats_row is not None:
            stats_row.copy_(net.grads[net.n_params:net.n_params + 2], non_blocking=True)

    def fit(self, batch, epochs, seed):
        """`epochs` passes over the pool's labelled rows in minibatches of `batch` (a short last one takes its mean over its own size),
        shuffled by a generator seeded with (seed, the steps taken so far): one int32 upload and one synchronisation per epoch.
        -> [(epoch, batch index, loss, metric per sample)]."""
        batch, epochs = int(batch), int(epochs)
        if batch < 1 or epochs < 0:
            raise ValueError("batch must be at least 1 and epochs at least 0, got %d and %d" % (batch, epochs))
        rows = self.pool.labelled_rows()
        if len(rows) < 1:
            raise ValueError("the demonstration pool holds no labelled row")
        batch = min(batch, len(rows))
        n_steps = -(-len(rows) // batch)
        pinned = torch.empty((n_steps, 2), dtype=torch.float32).pin_memory()
        log = []
        for epoch in range(1, epochs + 1):
            order = epoch_order(rows, seed, self.step_count)
            idx = torch.from_numpy(order).to(self.net.device)
            sizes = [min(batch, len(rows) - lo) for lo in range(0, len(rows), batch)]
            for k, size in enumerate(sizes):
                self.step(idx[k * batch:], size, pinned[k])
            torch.cuda.current_stream(self.net.device).synchronize()     # the one synchronisation of the epoch
            per = float(self.net.n_actions) if self.net.continuous else 1.0
            log += [(epoch, k, float(pinned[k, 0]), float(pinned[k, 1]) / (size * per)) for k, size in enumerate(sizes)]
        return log


def epoch_order(rows, seed, salt):
    """The shuffled int32 row indices of one epoch: numpy's PCG64 seeded with (seed, salt), so that an epoch depends on the seed and on
    how many steps came before it and on nothing else."""
    rng = np.random.Generator(np.random.PCG64([int(seed) & (2 ** 63 - 1), int(salt)]))
    return np.asarray(rows, np.int32)[rng.permutation(len(rows))]


def clone_actor(net, pool, lr, batch, epochs, seed, trainer=None):
    """GenericPPO.clone_actor: `epochs` passes of behaviour cloning over `pool`.  trainer: a CloneTrainer to go on with (its Adam
    moments and step counter persist); a fresh one otherwise.  Leaves ``net.clone_log`` and returns it."""
    trainer = CloneTrainer(net, pool, lr) if trainer is None else trainer
    if trainer.net is not net or trainer.pool is not pool:
        raise ValueError("the trainer was built for another net or pool")
    trainer.set_lr(lr)
    net.clone_log = trainer.fit(batch, epochs, seed)
    return net.clone_log
