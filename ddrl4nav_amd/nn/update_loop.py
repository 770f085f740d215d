"""The one update loop of every PPO learner (nn/ppo.py PPO.learn, nn/generic.py GenericPPO.learn): what a step reads, where an Atari
step's frames come from, and what follows a step's launch.

A Step is one optimiser step that a step source has prepared: its launcher and columns.  learn_columns() reads the columns out of a
batch.  The Atari sources are PPO._full_batch_steps (all knobs at their defaults: ONE step, handed out TRAINING_ITER_TIME times) and
minibatch.steps (epochs of K minibatches).  Both take their launchers from a frame source -- StackedFrames over uint8 [B, C, 84, 84],
PlaneFrames over data.FramePlanes -- which alone decides between the staged and the in-place form (config_nn.FRAMES_IN_PLACE) and
alone calls HotPath.ppo_iter / ppo_iter_indexed.  GenericPPO's source is one Step whose launcher runs its micro-batches.
run() owns everything after the launch: diagnostics, KL stop, gradient all-reduce, Adam step, statistics read-back, loss dict.  It
talks to the net's update backend (net.update_backend: engine.HotPath for PPO, GenericPPO itself) through set_rates, loss_options,
ppo_diag, diag_global, allreduce_grads, clip_adam_step, stats and, deferred only, stats_async.
"""
import collections
import time
from functools import partial

import torch

from ddrl4nav_amd import ops
from ddrl4nav_amd.data.frame_planes import FramePlanes
from ddrl4nav_amd.nn import minibatch

# launch(actions, old_logps, advs, rets, b_global=, old_values=) enqueues the step's ppo_iter on its frames; ppo_diag reads actions,
# old_logps, rets.  old_values: the collecting policy's values, the fifth column of a net with VALUE_CLIP (None otherwise)
Step = collections.namedtuple("Step", "launch actions old_logps advs rets b_global old_values", defaults=(None,))


def learn_columns(data, device, wants_old_values, n_extra_critics=0):
    """((actions, old_logps, advs, rets, old_values), extra_rets) of a batch: fp32, contiguous, on `device`.  Row 0 of data.values is the
    return target; with wants_old_values (VALUE_CLIP) row 1 is what the collecting policy predicted (not derivable: ret = fl(v_old + adv)
    is rounded), else old_values is None; with an extra critic (reference ppo.py:97-104) its targets are the LAST row, else extra_rets
    is empty."""
    f32 = lambda t: torch.as_tensor(t, dtype=torch.float32, device=device).contiguous()
    values = f32(data.values)
    old_values = None
    if wants_old_values:
        if values.dim() != 2 or values.shape[0] < 2:
            raise ValueError("VALUE_CLIP needs the collecting policy's values as row 1 of data.values (row 0: the returns); this "
                             "batch has %d row(s) -- the rollouts emit it for a net with VALUE_CLIP, the Redis learner path cannot "
                             "(its workers overwrite their values with the returns)" % (values.shape[0] if values.dim() == 2 else 1))
        old_values = values[1].contiguous()
    assert n_extra_critics == 0 or values.shape[0] >= 1 + n_extra_critics, "data.values needs one row per critic"
    extra_rets = [values[-1].contiguous()] if n_extra_critics else []
    return (f32(data.actions), f32(data.old_logps), f32(data.advs), values[0].contiguous(), old_values), extra_rets


class StackedFrames:
    """Frames uint8 [B, C, 84, 84] on the device.  stage: uint8 [>= n, C, 84, 84] that gathered() fills (staged); tab: int32 [>= n, 4]
    (in place).  Both methods return a launcher, the HotPath call with its frames bound; what they enqueue precedes it in stream order."""

    def __init__(self, hp, frames, in_place, stage=None, tab=None):
        self.hp, self.frames, self.in_place, self.stage, self.tab = hp, frames, in_place, stage, tab

    def contiguous(self, lo, hi):
        """Samples lo..hi-1 in storage order: a view, in place or not."""
        return partial(self.hp.ppo_iter, self.frames[lo:hi])

    def gathered(self, idx, n, columns, columns_dst, adv_affine):
        """The n samples idx names; the four float columns ride along into columns_dst (the advantages through adv_affine if given)."""
        if self.in_place:
            tab = ops.frame_table_stacks(self.frames, self.tab, idx=idx, n=n, columns=columns, columns_dst=columns_dst, adv_affine=adv_affine)
            return partial(self.hp.ppo_iter_indexed, self.frames, tab)
        ops.gather_minibatch(self.frames, idx, self.stage, columns, columns_dst, adv_affine=adv_affine, n=n)
        return partial(self.hp.ppo_iter, self.stage[:n])


class PlaneFrames(StackedFrames):
    """data.FramePlanes, every frame stored once: stacks are assembled into `stage`, or read where they lie through `tab`."""

    def contiguous(self, lo, hi):
        if self.in_place:
            return partial(self.hp.ppo_iter_indexed, self.frames.pool, self.frames.table(self.tab, first=lo, n=hi - lo))
        return partial(self.hp.ppo_iter, self.frames.stacks(lo, hi, out=self.stage))

    def gathered(self, idx, n, columns, columns_dst, adv_affine):
        if self.in_place:
            tab = self.frames.table(self.tab, idx=idx, n=n, columns=columns, columns_dst=columns_dst, adv_affine=adv_affine)
            return partial(self.hp.ppo_iter_indexed, self.frames.pool, tab)
        self.frames.gather(self.stage, idx, n=n, columns=columns, columns_dst=columns_dst, adv_affine=adv_affine)
        return partial(self.hp.ppo_iter, self.stage[:n])


def frame_source(hp, frames, in_place, stage=None, tab=None):
    return (PlaneFrames if isinstance(frames, FramePlanes) else StackedFrames)(hp, frames, in_place, stage, tab)


def run(net, steps, n_steps, deferred=False):
    """learn()'s protocol over the n_steps Steps of `steps`.  Eager: one host synchronisation per step, the weights match update_time at
    every yield (the reference's protocol).  deferred (PPO passes its deferred_stats, config_nn.DEFERRED_LOSS_READBACK; GenericPPO has no
    such path and passes nothing): every step is enqueued back to back,
    its statistics tail and diagnostics sums go to pinned host rows of their own by asynchronous copies, and ONE synchronisation
    precedes the yields -- same keys, values and update_time per yield, but the weights are already the last step's at the first yield
    (the reference's consumer, backward.py:189-209, publishes after the last one either way), and with N > 1 ranks a slow host does not
    stall the others' collectives once per step."""
    diag = net.diagnostics
    if net.target_kl is not None and deferred:   # net.deferred_stats switched on after construction
        raise ValueError("TARGET_KL needs the host after every step: not with DEFERRED_LOSS_READBACK (net.deferred_stats)")
    if deferred and (net._stats_rows is None or net._stats_rows.shape[0] < n_steps):
        net._stats_rows = torch.empty((n_steps, 8), dtype=torch.float32).pin_memory()
    if deferred and diag and (net._diag_rows is None or net._diag_rows.shape[0] < n_steps):
        # a device row per step as well: the next step must not overwrite what a copy still reads
        net._diag_rows = torch.empty((n_steps, ops.DIAG_SLOTS), dtype=torch.float64).pin_memory()
        net._diag_dev = torch.zeros((n_steps, ops.DIAG_SLOTS), dtype=torch.float64, device=net.device)
    t_all = t0 = time.time()
    for i, s in enumerate(steps):
        hp = net.update_backend   # read per step: the Atari step sources ensure the capacity, which may rebuild the hot path
        hp.loss_options = net.loss_options
        if net.lr_anneal is not None:
            # the rates of optimiser step number net.anneal_step (counted at enqueue: the deferred read-back sees the same numbers);
            # host arithmetic and four words of the context, no synchronisation
            hp.set_rates(*minibatch.annealed_rates(net._base_rates, net.anneal_step, *net.lr_anneal))
        s.launch(s.actions, s.old_logps, s.advs, s.rets, b_global=s.b_global, old_values=s.old_values)
        d = None
        if diag and deferred:
            net._diag_rows[i].copy_(hp.ppo_diag(s.actions, s.old_logps, s.rets, out=net._diag_dev[i]), non_blocking=True)
        elif diag:
            # read before anything is applied: the sums describe the policy this step's loss was evaluated with, combined over the
            # ranks so that every rank takes the same decision (one that stopped alone would leave the others in the all-reduce)
            d = ops.diag_dict(hp.diag_global(hp.ppo_diag(s.actions, s.old_logps, s.rets)))
            if ops.kl_stop(d, net.target_kl):
                return   # ends the whole call; this step is not applied: no all-reduce, no Adam, no yield, update_time as it was
        hp.allreduce_grads()
        hp.clip_adam_step()
        net.anneal_step += 1   # a step the KL stop skipped does not count
        if deferred:
            hp.stats_async(net._stats_rows[i])
            continue
        net.update_time += 1
        yield ops.loss_dict(hp.stats(), time.time() - t0, d), net.update_time, True   # one device->host copy
        t0 = time.time()
    if not deferred:
        return
    torch.cuda.current_stream().synchronize()   # the one synchronisation of the call
    dt = (time.time() - t_all) / max(n_steps, 1)
    for i in range(n_steps):
        net.update_time += 1
        # the ranks' diagnostics rows are combined after the synchronisation (a collective per step, on the host)
        d = ops.diag_dict(net.update_backend.diag_global(net._diag_rows[i])) if diag else None
        yield ops.loss_dict(ops.stats_dict(net._stats_rows[i]), dt, d), net.update_time, True
