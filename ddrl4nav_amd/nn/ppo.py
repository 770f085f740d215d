"""PPO: drop-in for USTC_lab.nn.PPO on the Pong / AtariPreNet path (reference ppo.py:17-146).

Same constructor arguments, same ``forward(states, act=None, play_mode=False)`` return shape,
same ``learn(data)`` generator protocol and loss-dict keys, same ``state_dict()`` key names and
nn2redis blob -- but every tensor op of the reference is replaced by the HIP kernels behind
include/ddrl.h.  The module's parameters are views into one flat fp32 arena (the reference's
named_parameters() order), which is what the kernels, the Adam step and the RCCL all-reduce use.  learn() is one loop over one of two
step sources, and one frame source decides where a step's frames are read (nn/update_loop.py).
"""
import torch

from ddrl4nav_amd.nn import minibatch
from ddrl4nav_amd.data import Experience
from ddrl4nav_amd.data.frame_planes import FramePlanes, planes_of
from ddrl4nav_amd.dist import global_batch
from ddrl4nav_amd.engine import HotPath
from ddrl4nav_amd.nn.base import Basenn, bind_arena
from ddrl4nav_amd.nn.distribution import HipCategorical
from ddrl4nav_amd.nn.update_loop import Step, frame_source, learn_columns, run


from ddrl4nav_amd.nn.atari_encoder import frames_u8 as _frames_u8  # noqa: E402


class PPO(Basenn):
    def __new__(cls, actor, critic, prenet=None, *args, **kwargs):
        """``PPO(...)`` over anything but the Atari encoder is the operator-composed GenericPPO
        (nn/generic.py): same constructor, same protocol."""
        from ddrl4nav_amd.nn.atari_encoder import AtariPreNet
        enc = prenet if prenet is not None else getattr(actor, "pre", None)
        if cls is PPO and not isinstance(enc, AtariPreNet):
            from ddrl4nav_amd.nn.generic import GenericPPO
            return GenericPPO(actor, critic, prenet, *args, **kwargs)
        return super().__new__(cls)

    def __init__(self, actor, critic, prenet=None, rnd=None, config=None, config_nn=None, max_batch=None,
                 process_group=None):
        super().__init__(config, config_nn)
        # the optional knobs of config_nn, all read in nn/minibatch.py learner_options.  PPO_DIAGNOSTICS / TARGET_KL: ApproxKL,
        # ClipFraction, ExplainedVariance and RatioMax in every loss dict, and KL early stopping.  PPO_MINIBATCHES / PPO_SHUFFLE /
        # NORMALIZE_ADVANTAGE / ADV_NORM_EPS: epochs of minibatch steps.  FRAMES_IN_PLACE: no batch or minibatch of frames is
        # materialised, the conv1 kernels read them where they lie through a frame table (ddrl_ppo_iter_indexed).  ACT_IN_PLACE: a
        # PlaneRollout over this net acts on its pool in place.  VALUE_CLIP / ENTROPY_BONUS_SPLIT: the loss block's option form
        # (ddrl_ppo_iter_opt).  LR_ANNEAL_UPDATES / LR_ANNEAL_FLOOR / CLIP_ANNEAL: linear schedules of the rates (ddrl_set_rates)
        (self.diagnostics, self.target_kl, self.minibatch, self.frames_in_place, self.act_in_place, self.loss_options, self.lr_anneal,
         self._base_rates) = minibatch.learner_options(config_nn)
        self.anneal_step = 0       # optimiser steps this net has applied: the schedule's u
        self._frame_tab = None      # FramePlanes states, full-batch step, in place: int32 [B, 4]
        self._mb_stage = None
        self._plane_batch = None   # FramePlanes states, full-batch step, staged: the batch materialised once per learn call
        self.learn_calls = 0   # learn() calls with a minibatch knob set: the second integer of minibatch.epoch_order
        if hasattr(actor, "log_std"):
            raise NotImplementedError("the Atari fast path has a Categorical actor only (reference atari.yaml)")
        if bool(config_nn.SHARE_CNN_NET) != (prenet is not None):
            raise ValueError("SHARE_CNN_NET=True needs a shared prenet (and pre-less actor / critic); "
                             "SHARE_CNN_NET=False needs prenet=None (reference runner/utils.py:122-143)")
        if rnd is not None:
            raise NotImplementedError("RND is disabled in the reference defaults (USE_RND=False) and out of scope")
        self.device = torch.device(config.DEVICE if str(config.DEVICE) != "cuda" else "cuda:%d" % torch.cuda.current_device())
        self.prenet = prenet
        self.actor = actor
        self.critic = critic
        self._critics = [self.critic]
        self.rnd = rnd
        self.gail_critic = False
        self.share_cnn_net = config_nn.SHARE_CNN_NET
        self.training_iter_time = config_nn.TRAINING_ITER_TIME
        self.update_time = 0
        self._cfg_nn = config_nn
        self._process_group = process_group
        self._seed = int(torch.initial_seed()) & (2 ** 63 - 1)
        self._calls = 0
        self._hp = None
        # learn(): False = one host sync per iteration (the reference's protocol: weights match update_time at every yield);
        # True = all iterations enqueued, one sync, then the yields (config_nn.DEFERRED_LOSS_READBACK; bench.py sets it)
        self.deferred_stats = bool(getattr(config_nn, "DEFERRED_LOSS_READBACK", False))
        self._stats_rows = None
        self._diag_rows = self._diag_dev = None
        n_actions = actor.action_output_dim
        in_ch = (prenet if prenet is not None else actor.pre).conv1.in_channels
        cap = int(max_batch if max_batch is not None else max(2 * config_nn.TRAINING_MIN_BATCH, 2048))
        self._build(cap, n_actions, in_ch)
        actor._bind_owner(self)    # net.actor(x) / net.critic(x) as the reference offers them (actor.py:27-40, critic.py:14-21)
        critic._bind_owner(self)

    # ---- arena binding --------------------------------------------------------------------------
    def _hot_path_kwargs(self):
        c = self._cfg_nn
        return dict(share_cnn_net=1 if c.SHARE_CNN_NET else 0, learning_rate=float(c.LEARNING_RATE),
                    smooth_l1_loss=1 if c.SMOOTH_L1_LOSS else 0, clip_grad=1 if c.CLIP_GRID else 0, clip_grad_norm=float(c.CLIP_GRID_NUM),
                    actor_lr=float(c.ACTOR_LEARNING_RATE), critic_lr=float(c.CRITIC_LEARNING_RATE),
                    ppo_clip=float(c.PPO_CLIP), dual_clip=float(c.DUEL_PPO_CLIP), v_loss_theta=float(c.V_LOSS_THETA),
                    ent_loss_theta=float(c.ENTROPY_LOSS_THETA))

    def _build(self, max_batch, n_actions, in_ch, old=None):
        hp = HotPath(max_batch=max_batch, device=self.device, n_actions=n_actions, in_channels=in_ch,
                     process_group=self._process_group, **self._hot_path_kwargs())
        params = list(self.named_parameters())
        total = sum(p.numel() for _, p in params)
        if total != hp.n_params:
            raise ValueError("module tree has %d parameters, the HIP path expects %d" % (total, hp.n_params))
        bind_arena(params, hp.params)
        if old is not None:
            hp.adam_m.copy_(old.adam_m)
            hp.adam_v.copy_(old.adam_v)
            from ddrl4nav_amd._lib import check
            check(hp.lib.ddrl_set_step(hp.ctx, old.step))
            old.close()
        hp.params_changed()
        self._hp = hp

    def _ensure_capacity(self, n):
        if n > self._hp.max_batch:
            self._build(int(n), self._hp.n_actions, int(self._hp.cfg.in_channels), old=self._hp)

    @property
    def hot_path(self):
        return self._hp

    update_backend = hot_path   # what nn/update_loop.py run() drives

    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._hp.params_changed()
        return out

    def params_changed(self):
        """Rebuild the packed weight layouts after an in-place write to the parameter views."""
        if self._hp is not None:
            self._hp.params_changed()

    def to(self, *args, **kwargs):  # the arena already lives on the GPU; keep `.to(DEVICE)` callers happy
        return self

    # ---- PPO.forward (ppo.py:72-75) ----------------------------------------------------------------
    def forward(self, states, act=None, play_mode=False):
        frames = _frames_u8(states, self.device)
        n = frames.shape[0]
        self._ensure_capacity(n)
        self._calls += 1
        a_in = None if act is None else torch.as_tensor(act, dtype=torch.float32, device=self.device).contiguous()
        probs, value, action, logp = self._hp.forward(frames, act=a_in, seed=self._seed, stream_id=self._calls)
        values = [value.view(n, 1)]
        if play_mode:
            return (probs, logp if act is not None else None), values
        if act is None:
            dist = HipCategorical(self._hp, probs, self._seed, self._calls, action, logp)
            return (dist, None), values
        dist = HipCategorical(self._hp, probs, self._seed, self._calls, a_in, logp)
        return (dist, logp), values

    def add_critic(self, critic):
        raise NotImplementedError("extra critics (RND / GAIL) are out of scope on this path")

    def get_rnd(self, states):
        raise NotImplementedError("RND is out of scope on this path")

    def states_normalization(self, states):
        return states / 255

    # ---- PPO.learn (ppo.py:77-146) -----------------------------------------------------------------
    @property
    def wants_old_values(self):
        """True when learn() needs data.values row 1, the collecting policy's values (VALUE_CLIP): a rollout's batch() then emits it."""
        return self.loss_options[0] > 0.0

    def _full_batch_steps(self, frames, columns, old_values=None):
        """The step source with every minibatch knob at its default: ONE step over the whole batch, prepared once per learn call and
        handed out TRAINING_ITER_TIME times.  Stacked frames are read as they are.  FramePlanes are materialised into _plane_batch (for
        the length of learn() the batch holds the stacked size again: the plane pool's saving lasts through the update only with
        minibatch epochs or in place) or, with FRAMES_IN_PLACE, tabled into _frame_tab and read where they lie."""
        B = len(frames)
        self._ensure_capacity(B)
        if isinstance(frames, FramePlanes) and self.frames_in_place:
            if self._frame_tab is None or self._frame_tab.shape[0] < B:
                self._frame_tab = torch.empty((B, 4), dtype=torch.int32, device=self.device)
        elif isinstance(frames, FramePlanes):
            if self._plane_batch is None or self._plane_batch.shape[0] < B or tuple(self._plane_batch.shape[1:]) != frames.shape[1:]:
                self._plane_batch = torch.empty(frames.shape, dtype=torch.uint8, device=self.device)
        launch = frame_source(self._hp, frames, self.frames_in_place, self._plane_batch, self._frame_tab).contiguous(0, B)
        # data-parallel: every rank scales by 1 / (sum of the ranks' batch sizes) -- shards may be uneven
        step = Step(launch, *columns, global_batch(B, self._process_group), old_values)
        for _ in range(self.training_iter_time):
            yield step

    def learn(self, data: Experience):
        """One loop (nn/update_loop.py run()) over one of two step sources: the single full-batch step above, or, with a minibatch knob
        set, TRAINING_ITER_TIME epochs of K steps (nn/minibatch.py steps())."""
        (*columns, old_values), _ = learn_columns(data, self.device, self.wants_old_values)
        fp = planes_of(data.states)
        frames = fp if fp is not None else _frames_u8(data.states, self.device)
        assert columns[3].shape == (len(frames),)
        if self.minibatch != minibatch.DEFAULTS:
            steps, n_steps = minibatch.steps(self, frames, columns, old_values), self.training_iter_time * self.minibatch[0]
        else:
            steps, n_steps = self._full_batch_steps(frames, columns, old_values), self.training_iter_time
        yield from run(self, steps, n_steps, self.deferred_stats)
