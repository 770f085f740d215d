"""Imitation pre-training: behaviour cloning of the Atari actor from demonstrated (state, action) pairs, on the device.

Stands in for ``Basenn._imitation_learning_classifier`` (USTC_lab/nn/base.py:120-150), which ``BackwardTrainThread.run`` calls before
PPO begins when ``MIMIC_START`` is set (server/backward.py:117-129,168-174).  The reference's expression
``criterion(self(X), Y)`` cannot run on a PPO net (``PPO.forward`` returns a tuple, the reader's labels are float32 [n, 1]) and its
regression variant is an empty ``pass``; what is built here is the computation it intends:

  * ``loss = F.cross_entropy(actor_linear(pre(x)), y.long())`` on the pre-softmax logits, the mean over the batch (a short last batch
    over its own size);
  * a fresh ``Adam(lr=imitation_learning_rate)`` with torch's defaults and no gradient clipping, with its own m / v / step counter;
  * only the actor's encoder (``actor.pre`` or the shared ``prenet``) and ``actor_linear`` get a gradient; torch's Adam skips
    parameters whose gradient is None, so the critic side and the PPO optimiser's state stay bit-unchanged;
  * ``nn2redis(pipe, update_key, imitation_model_key)`` after every ``imitation_saving_frequency`` epochs.

Per batch: ddrl_op_gather_rows_u8 (the whole demonstration set lives on the device as uint8; an epoch's shuffle costs one int32 upload)
-> ddrl_encoder_forward -> ddrl_op_heads_bc_loss -> ddrl_encoder_backward -> ddrl_op_clip_adam, on an encoder-only context bound to the
actor side's slice of the parameter arena with a private gradient buffer and workspace.  No host synchronisation per batch: every
batch's (loss, correct) goes to a pinned row; one synchronisation per epoch, then the reference's per-batch log lines.
"""
import logging
from ctypes import byref, c_int64, c_void_p

import numpy as np
import torch

from ddrl4nav_amd import _lib, ops
from ddrl4nav_amd._lib import STATS_FLOATS, check
from ddrl4nav_amd.ops import _p, _st
from ddrl4nav_amd.nn.atari_encoder import frames_u8

FEAT = 512
KWARGS = ("imitation_learning_rate", "imitation_training_batch", "imitation_training_epoch", "imitation_saving_frequency",
          "imitation_model_key", "imitation_training_type")


def validate_labels(labels, n_actions):
    """The demonstrated actions as a float32 [N] host array; ValueError unless every one is an integer in [0, n_actions)."""
    y = np.asarray(labels, dtype=np.float64).reshape(-1)
    bad = ~(np.isfinite(y) & (y >= 0) & (y < n_actions) & (y == np.floor(y)))
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError("demonstration label %r of sample %d is not an action index in [0, %d)" % (float(y[i]), i, n_actions))
    return y.astype(np.float32)


def check_supported(net, training_type):
    """NotImplementedError, naming the reason, for everything the reference gives no runnable meaning to."""
    from ddrl4nav_amd.nn.ppo import PPO
    if training_type == "regression":
        raise NotImplementedError("imitation_training_type='regression': the reference's regression body is an empty `pass` "
                                  "(nn/base.py:117-118); only 'classification' is built")
    if training_type != "classification":
        raise ValueError("imitation_training_type must be 'classification' or 'regression', got %r" % (training_type,))
    actor = getattr(net, "actor", None)
    if actor is not None and hasattr(actor, "log_std"):
        raise NotImplementedError("imitation pre-training needs a Categorical actor: the reference's classification reader is registered "
                                  "for atari only (data/mimic_exp.py reader_register) and a Gaussian actor has no class logits")
    if not isinstance(net, PPO):
        raise NotImplementedError("imitation pre-training is built for the Atari PPO net only (%s: the reference's classification "
                                  "reader is registered for atari only, data/mimic_exp.py reader_register)" % type(net).__name__)


def actor_prefix(net):
    """(encoder floats, prefix floats): the actor side -- its encoder, then actor_linear -- must be the PREFIX of the flat arena in
    named_parameters() order, in both SHARE_CNN_NET modes (actor.pre.* or prenet.*, then actor.actor_linear.*)."""
    enc = "prenet." if net.prenet is not None else "actor.pre."
    want = [enc + l + "." + t for l in ("conv1", "conv2", "conv3", "linear") for t in ("weight", "bias")]
    want += ["actor.actor_linear.weight", "actor.actor_linear.bias"]
    params = list(net.named_parameters())
    base, off, enc_floats = net.hot_path.params.data_ptr(), 0, 0
    for i, name in enumerate(want):
        if i >= len(params) or params[i][0] != name or params[i][1].data_ptr() != base + 4 * off:
            raise ValueError("the actor side (%s*, actor.actor_linear.*) is not the prefix of the parameter arena: parameter %d is %r, "
                             "expected %r at float offset %d" % (enc, i, params[i][0] if i < len(params) else None, name, off))
        off += params[i][1].numel()
        if i == 7:
            enc_floats = off
    return enc_floats, off


class ImitationTrainer:
    """The device side of one ``imitation_learning`` call: the encoder-only context over the actor prefix, the private gradient /
    Adam buffers and the step."""

    def __init__(self, net, batch, lr):
        hp = net.hot_path
        self.net, self.hp, self.lib = net, hp, hp.lib
        self.device, self.cap, self.A = hp.device, int(batch), hp.n_actions
        self.enc_floats, self.prefix = actor_prefix(net)
        C = int(hp.cfg.in_channels)
        f32 = dict(dtype=torch.float32, device=self.device)
        self._cfg = _lib.default_config(max_batch=self.cap, n_actions=self.A, in_channels=C, share_cnn_net=1)
        n_ctx, n_act, wb, ab = c_int64(), c_int64(), c_int64(), c_int64()
        check(self.lib.ddrl_param_count(byref(self._cfg), byref(n_ctx), byref(n_act)))
        check(self.lib.ddrl_workspace_bytes(byref(self._cfg), byref(wb)))
        check(self.lib.ddrl_op_clip_adam_ws_bytes(byref(ab)))
        with torch.cuda.device(self.device):
            # private: gradients of the prefix + the statistics tail (stats of the loss head at [prefix, prefix + 2), the optimiser's
            # norm behind them); sized for the context's own layout, of which the encoder slots are written
            self.grads = torch.zeros(max(self.prefix, n_ctx.value) + STATS_FLOATS, **f32)
            self.m = torch.zeros(self.prefix, **f32)
            self.v = torch.zeros(self.prefix, **f32)
            self._workspace = torch.empty(wb.value, dtype=torch.uint8, device=self.device)
            self._adam_ws = torch.empty(ab.value, dtype=torch.uint8, device=self.device)
            self._bc_ws = torch.empty(ops.heads_bc_ws_floats(self.A, self.cap), **f32)
            self.frames = torch.empty((self.cap, C, 84, 84), dtype=torch.uint8, device=self.device)
            self.labels = torch.empty(self.cap, **f32)
        if hp.params.data_ptr() % 16 or self.grads.data_ptr() % 16:
            raise ValueError("the parameter / gradient arenas must be 16-byte aligned")
        ctx = c_void_p()
        check(self.lib.ddrl_ctx_create(byref(self._cfg), _p(hp.params), _p(self.grads), _p(None), _p(None), _p(self._workspace), wb.value,
                                       byref(ctx)))
        self.ctx = ctx
        h, dh = c_void_p(), c_void_p()
        check(self.lib.ddrl_encoder_buffers(ctx, byref(h), byref(dh)))
        w32 = self._workspace.view(torch.float32)
        view = lambda ptr: w32[(ptr.value - self._workspace.data_ptr()) // 4:][:self.cap * FEAT].view(self.cap, FEAT)
        self.h, self.dh = view(h), view(dh)
        # the optimiser's configuration: one group over the prefix, no clipping (the reference's Adam(self.parameters(), lr))
        self._opt_cfg = _lib.default_config(max_batch=self.cap, n_actions=self.A, in_channels=C, share_cnn_net=1, clip_grad=0,
                                            learning_rate=float(lr))
        self.step_count = 0
        check(self.lib.ddrl_params_changed(self.ctx))

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.ddrl_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, frames_all, labels_all, idx, n, stats_row=None):
        """One optimiser step on the n samples frames_all[idx[:n]] (everything on the device, nothing waits for the host);
        stats_row: a pinned [2] host row that receives (loss, correct) asynchronously."""
        lib, p, g = self.lib, self.hp.params, self.grads
        st = _st()
        wo, bo = self.enc_floats, self.enc_floats + self.A * FEAT
        ops.gather_rows_u8(frames_all, idx, self.frames, labels_all, self.labels, n)
        check(lib.ddrl_encoder_forward(self.ctx, _p(self.frames), n, st))
        ops.heads_bc_loss(p[wo:], p[bo:], self.A, self.h, FEAT, n, self.labels, n, self.dh, FEAT, g[wo:], g[bo:], g[self.prefix:],
                          self._bc_ws)
        check(lib.ddrl_encoder_backward(self.ctx, _p(self.frames), n, st))
        self.step_count += 1
        check(lib.ddrl_op_clip_adam(byref(self._opt_cfg), _p(p), _p(g), _p(self.m), _p(self.v), self.prefix, self.prefix, 1, self.step_count,
                                    _p(self._adam_ws), st))
        check(lib.ddrl_params_changed(self.ctx))     # this context's packed encoder weights follow every step
        if stats_row is not None:
            stats_row.copy_(g[self.prefix:self.prefix + 2], non_blocking=True)


def imitation_learning(net, dataset, pipe, update_key, **kwargs):
    """``Basenn.imitation_learning(dataset, pipe, update_key, **kwargs)`` for the Atari PPO net; kwargs as the reference's learner
    passes them (server/backward.py:122-129).  Leaves ``net.imitation_log`` = [(epoch, batch_index, loss, accuracy), ...]."""
    from ddrl4nav_amd.data.mimic_exp import batches
    missing = [k for k in KWARGS if k not in kwargs]
    if missing:
        raise TypeError("imitation_learning: missing keyword arguments %s" % ", ".join(missing))
    check_supported(net, kwargs["imitation_training_type"])
    batch, epochs = int(kwargs["imitation_training_batch"]), int(kwargs["imitation_training_epoch"])
    freq, key = int(kwargs["imitation_saving_frequency"]), kwargs["imitation_model_key"]
    if batch < 1 or freq < 1:
        raise ValueError("imitation_training_batch and imitation_saving_frequency must be positive")
    hp = net.hot_path
    N = len(dataset)
    if N < 1:
        raise ValueError("the demonstration data set is empty")
    items = [dataset[i] for i in range(N)]
    labels_host = validate_labels([np.asarray(y).reshape(-1)[0] for _, y in items], hp.n_actions)   # before anything is uploaded
    batch = min(batch, N)
    frames_all = frames_u8(np.stack([np.asarray(x) for x, _ in items]), hp.device)
    del items
    C = int(hp.cfg.in_channels)
    if tuple(frames_all.shape[1:]) != (C, 84, 84):
        raise ValueError("demonstration states are %s, the net takes [%d, 84, 84]" % (tuple(frames_all.shape[1:]), C))
    labels_all = torch.from_numpy(labels_host).to(hp.device)
    loader = batches(dataset, batch)
    trainer = ImitationTrainer(net, batch, kwargs["imitation_learning_rate"])
    rows = torch.empty((len(loader), 2), dtype=torch.float32).pin_memory()
    net.imitation_log = []
    try:
        for epoch in range(1, epochs + 1):
            logging.info("======================================\n")
            logging.info("training epoches : {}".format(epoch))
            logging.info("======================================\n")
            chunks = list(loader.iter_indices())
            order = torch.tensor([i for c in chunks for i in c], dtype=torch.int32).to(hp.device)   # the epoch's whole permutation: one upload
            lo = 0
            for k, c in enumerate(chunks):
                trainer.step(frames_all, labels_all, order[lo:lo + len(c)], len(c), rows[k])
                lo += len(c)
            torch.cuda.current_stream().synchronize()   # the one synchronisation of the epoch
            for k, c in enumerate(chunks):
                loss, correct = float(rows[k, 0]), float(rows[k, 1])
                logging.info("Batch_Index = {}, Loss = {}".format(k, loss))
                net.imitation_log.append((epoch, k, loss, correct / len(c)))
            if epoch % freq == 0:
                hp.params_changed()
                if pipe is not None:
                    net.nn2redis(pipe, update_key, key)
    finally:
        hp.params_changed()     # the net's own packed weights follow the arena, whatever happened
        trainer.close()
