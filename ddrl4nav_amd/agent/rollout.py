"""DeviceRollout: the device-resident experience pool that replaces the per-step Experience
records + Redis training blobs of the reference (agent.py:217-296, multiqueue.py:83-105,
backward.py:48-62) when Forward, Env bookkeeping and Backward are co-located on one GPU.

Pool layout (all on the GPU, [time][env] major so that GAE loads are coalesced across envs):
  frames  uint8 [T+1, N, C, 84, 84]    values f32 [T+1, N]     rewards f32 [T, N]
  actions f32 [T, N]   logps f32 [T, N]   dones u8 [T, N]      adv / ret f32 [T, N]
Frames arrive either as device tensors or through a pinned-host ring (data/ring.py) with
hipMemcpyAsync on a copy stream, overlapping the previous step's forward.  A slot is filled either with the whole stack
(put_frames*) or from ONE new frame per env (put_new_frames*): csrc/fstack.hip then builds slot t from slot t-1 on the device,
as the reference's FrameStackWrapper does on the host, and a quarter of the bytes cross PCIe at C = 4.

One core: everything but the observation -- the step pools, the counters, record() / finish() / carry_over(), the learner columns of
batch() and the ordering of the copy stream -- is _RolloutBase, shared by DeviceRollout, PlaneRollout (agent/plane_rollout.py) and
StateRollout.  Every ring-fed put follows one rule (_RolloutBase._order_copy_stream): the first of them after construction or after a
finish(), at whatever slot, makes the copy stream wait for the compute stream once; none waits after it.

Carry-over between rollouts (reference agent.py:286-292: ``rewards_step[0] = rewards_step[T]; exps = [exps[-1]]``): the
reference keeps the WHOLE (T+1)-th Experience -- state, the action already sent to the env, its old log-prob, its value
under the weights of that moment, its reward and done -- as step 0 of the next rollout and acts from step 1 on.
``carry_over(keep_step=True)`` does exactly that (rows T of every pool, which ``bootstrap()`` / ``record(T, ...)`` fill,
move to row 0; the next rollout starts at ``t0 == 1``).  The default, ``carry_over()``, carries the FRAME only and lets
``act(0)`` re-evaluate it with the current weights (a fresh action, log-prob and value for slot 0): a deviation from the
reference, listed in DESIGN.md section 7 -- it needs no env step between ``bootstrap()`` and ``finish()`` and its slot-0
sample is on-policy for the weights the update starts from."""
import torch

from ddrl4nav_amd.agent.agent import gae_device
from ddrl4nav_amd.agent.normalize import ReturnNorm, RunningNorm, check_knobs, obs_norm_flags
from ddrl4nav_amd.agent.statistics import EpisodeReturns, NavStatus
from ddrl4nav_amd.data import Experience
from ddrl4nav_amd.ops import file_flagged_rows, frame_stack_push, gae_bootstrap
from ddrl4nav_amd.utils.staging import copy_into


def value_rows(ret, values, T, B, with_old_values):
    """Experience.values of a rollout's batch: row 0 the return targets (a view of `ret`); for a net that clips its value loss
    (net.wants_old_values, VALUE_CLIP) also row 1, the T rows of values the collecting policy predicted (a copy: carry_over rewrites
    values[0])."""
    if not with_old_values:
        return ret.view(1, B)
    return torch.stack([ret.view(B), values[:T].reshape(B)])


class _RolloutBase:
    """What DeviceRollout, PlaneRollout and StateRollout share, written once: the [T+1, N] step pools and their [:T] views, adv / ret, the
    counters, the copy stream, record() / finish() / carry_over(), the learner columns of batch() and the ring-ordering rule.  A subclass
    adds its observation pool, its puts, act() and the `states` of batch(), and two hooks: _before_gae() and _carry_observation().

    normalize_returns (agent/normalize.py ReturnNorm): off (the default) nothing is allocated, nothing is launched
    and finish() runs GAE on the raw rewards as before."""
    ret_norm = None
    rewards_norm = None
    S = 0           # StateRollout(bootstrap_truncated=S): the depth of the pools of terminal observations; 0 = off

    def __init__(self, net, n_envs, horizon, gamma, landa, device, action_shape=None, track_returns=False, track_nav_status=False,
                 normalize_returns=False, reward_clip=10.0, norm_eps=1e-8):
        """action_shape: (T+1, N) (the default), or (T+1, N, n_actions) for a continuous net."""
        check_knobs(norm_eps, reward_clip)
        self.with_old_values = bool(getattr(net, "wants_old_values", False))
        self.N, self.T = N, T = int(n_envs), int(horizon)
        self.gamma, self.landa = gamma, landa
        self.device = dev = torch.device(device)
        f = dict(dtype=torch.float32, device=dev)
        self.values = torch.zeros((T + 1, N), **f)
        # rows 0..T-1 are the rollout (contiguous [T, N] views: what GAE and the learner batch read); row T holds the (T+1)-th
        # step's reward / done / action / log-prob for carry_over(keep_step=True)
        self._rewards = torch.zeros((T + 1, N), **f)
        self._dones = torch.zeros((T + 1, N), dtype=torch.uint8, device=dev)
        self._actions = torch.zeros((T + 1, N) if action_shape is None else action_shape, **f)
        self._logps = torch.zeros((T + 1, N), **f)
        self.rewards, self.dones = self._rewards[:T], self._dones[:T]
        self.actions, self.logps = self._actions[:T], self._logps[:T]
        self.adv = torch.empty((T, N), **f)
        self.ret = torch.empty((T, N), **f)
        self.t0 = 0        # first step the next rollout has to act on: 1 after carry_over(keep_step=True), else 0
        self.rollouts = 0  # finish() counts them (runner/device_loop.py resets its env before the first)
        self.copy_stream = torch.cuda.Stream(device=dev)
        self._ring_rollout = -1   # the rollout (self.rollouts) whose first ring-fed put ordered the copy stream
        self.returns = EpisodeReturns(N, dev) if track_returns else None
        self.nav_status = NavStatus(N, dev) if track_nav_status else None
        self._infos = torch.zeros((T + 1, N), dtype=torch.int32, device=dev) if track_nav_status else None
        if normalize_returns:
            self.ret_norm = ReturnNorm(N, T, gamma, dev, eps=norm_eps, clip=reward_clip)
            self.rewards_norm = self.ret_norm.rewards_norm

    def _order_copy_stream(self):
        """The one ring rule: the FIRST ring-fed put after construction or after a finish(), of whatever kind,
        slot and component, makes the copy stream wait for the current stream once, before its DMA -- whatever was enqueued there on the
        pools before this rollout (their zero fill, the previous update still reading them, carry_over(), an in-place normalisation)
        is through before the first DMA overwrites a slot.  No later put of that rollout waits again, so copy t + 1 runs under
        forward t (bench.py async_ingest_leg: waiting per slot cost 10 % of the overlapped ingest rate)."""
        if self._ring_rollout != self.rollouts:     # finish() counts the rollouts: one wait per rollout, none per slot
            self.copy_stream.wait_stream(torch.cuda.current_stream())
            self._ring_rollout = self.rollouts

    def record(self, t, rewards, dones, info=None, final_obs=None):
        """Reward / done of step t (0..T; T = the (T+1)-th step, only needed for keep_step); for a rollout that tracks the navigation
        status or bootstraps truncated episodes also the env's info words, and for the latter the env's terminal observations of the
        step (final_obs: [N, ...] fp32 device tensors, one per component), whose truncated rows are filed (_file_final_obs)."""
        if t < self.t0:
            raise ValueError("step %d was carried over from the previous rollout with its reward and done" % t)
        S = getattr(self, "S", 0)
        if S == 0 and final_obs is not None:
            raise ValueError("this rollout does not bootstrap truncated episodes: build it with bootstrap_truncated=S")
        if S > 0 and (info is None or final_obs is None):
            raise ValueError("this rollout bootstraps truncated episodes: record() needs the env's info words and its terminal "
                             "observations (an env built with emit_final_obs=True)")
        if self._infos is not None:
            if info is None:
                raise ValueError("this rollout tracks the navigation status: record() needs the env's info words")
            copy_into(self._infos[t], info)
        copy_into(self._rewards[t], rewards)
        copy_into(self._dones[t], dones)
        if S > 0:
            self._file_final_obs(t, final_obs)

    def _before_gae(self):
        """finish(): what a subclass commits in front of GAE (StateRollout: the observation statistics)."""

    def _gae(self):
        """finish(): GAE over rows 0..T-1, on the scaled rewards when normalize_returns is on.  Those rows are every step exactly once,
        also with carry_over(keep_step=True) (row T becomes row 0 of the next rollout), as for EpisodeReturns; the raw rewards stay.
        Under an initialised process group the commit of the return statistics is an all-reduce (through the host on gloo): finish()
        is then a synchronising collective that every rank has to call."""
        rewards = self.rewards if self.ret_norm is None else self.ret_norm.scale(self.rewards, self.dones)
        gae_device(self.values, rewards, self.dones, self.gamma, self.landa, adv=self.adv, ret=self.ret)

    def finish(self):
        """GAE over the rollout; with normalize_obs / normalize_returns first the commits of the statistics.  Under an initialised
        process group every commit is one small all-reduce (through the host on gloo): finish() is then a synchronising collective that
        EVERY rank has to call, once per normalised component and once for the returns, in this order."""
        self._before_gae()
        self._gae()
        if self.returns is not None:  # Status.update_reward_status over rows 0..T-1: every step once, also with keep_step
            self.returns.update(self.rewards, self.dones)
        if self.nav_status is not None:    # Status.update_nav_status over the same rows
            self.nav_status.update(self._infos[:self.T])
        self.rollouts += 1

    def carry_over(self, keep_step=False):
        """The last stored step becomes step 0 of the next rollout (agent.py:286-292).  keep_step=True: the whole step, as the
        reference keeps it (observation, action, old log-prob, value, reward, done of row T; the next rollout acts from t0 = 1);
        False (default): the observation only, slot 0 is evaluated again by act(0) under the current weights.  The observation moves
        as it is stored: a frame with its history (PlaneRollout), a slot normalised at its put (StateRollout)."""
        T = self.T
        if keep_step and self.S > 0:
            raise ValueError("carry_over(keep_step=True) is not supported with bootstrap_truncated: the terminal observation of row T "
                             "would have to move between rollouts")
        self._carry_observation()
        if keep_step:
            for pool in (self.values, self._rewards, self._dones, self._actions, self._logps, self._infos):
                if pool is not None:
                    pool[0].copy_(pool[T])
        self.t0 = 1 if keep_step else 0

    def _value_rows(self, B):
        return value_rows(self.ret, self.values, self.T, B, self.with_old_values)

    def _columns(self, B):
        """The learner's columns of batch() next to `states`: zero-copy views of rows 0..T-1."""
        return dict(advs=self.adv.view(B), actions=self.actions.view((B,) + tuple(self.actions.shape[2:])),
                    old_logps=self.logps.view(B), values=self._value_rows(B))

    def state_dict(self):
        """The running statistics a checkpoint has to carry next to the net's (host tensors): the return scaling's state and carry."""
        return {"ret_norm": None if self.ret_norm is None else self.ret_norm.state_dict()}

    def load_state_dict(self, sd):
        if (sd.get("ret_norm") is None) != (self.ret_norm is None):
            raise ValueError("normalize_returns differs between the saved rollout and this one")
        if self.ret_norm is not None:
            self.ret_norm.load_state_dict(sd["ret_norm"])


class DeviceRollout(_RolloutBase):
    def __init__(self, net, n_envs, horizon=256, channels=4, gamma=0.99, landa=0.95, device=None, seed=0, track_returns=False,
                 normalize_returns=False, reward_clip=10.0, norm_eps=1e-8):
        self.hp = net.hot_path if hasattr(net, "hot_path") else net
        super().__init__(net, n_envs, horizon, gamma, landa, device if device is not None else self.hp.device,
                         track_returns=track_returns, normalize_returns=normalize_returns, reward_clip=reward_clip, norm_eps=norm_eps)
        self.C = int(channels)
        self._probs = torch.empty((self.N, self.hp.n_actions), dtype=torch.float32, device=self.device)
        self.seed, self.t = int(seed), 0
        # single-frame ingest (put_new_frames*): allocated at first use, a host that ships whole stacks pays nothing
        self._newest = None                # uint8 [3, N, 84, 84]: 0 / 1 the ring's DMA targets (step parity), 2 put_new_frames' copy
        self._reset_buf = None             # uint8 [2, N]: 0 a caller's reset flags brought to the device, 1 all ones (reset=True)
        self._pushed = [None, None]        # events: the push kernel that read _newest[parity] is through
        self._alloc_observation()

    def _alloc_observation(self):
        self.frames = torch.empty((self.T + 1, self.N, self.C, 84, 84), dtype=torch.uint8, device=self.device)

    # ---- ingest ---------------------------------------------------------------------------------
    def put_frames(self, t, frames):
        """Device (or pinned host) uint8 frames [N,C,84,84] -> pool slot t."""
        copy_into(self.frames[t], frames)

    def put_frames_from_ring(self, t, ring):
        """hipMemcpyAsync from the pinned ring on the copy stream; the compute stream waits on it.  The FIRST ring-fed put of a rollout,
        at whatever t (slot 1 after the default carry_over(), which leaves t0 == 0), also orders the copy stream behind the compute
        stream (_order_copy_stream); later slots do not wait again."""
        self._order_copy_stream()
        ring.pop_to(self.frames[t], stream=self.copy_stream)
        torch.cuda.current_stream().wait_stream(self.copy_stream)

    def _single_frame_buffers(self):
        if self._newest is None:
            self._newest = torch.empty((3, self.N, 84, 84), dtype=torch.uint8, device=self.device)
            self._reset_buf = torch.ones((2, self.N), dtype=torch.uint8, device=self.device)
        return self._newest

    def _reset_flags(self, t, reset):
        """Checks (t, reset) of a single-frame put and returns the device flags [N] (or None).  reset: None = the dones recorded for step
        t-1, True = every env, False = none, else flags [N] (non-zero = reset)."""
        if t < self.t0:
            raise ValueError("step %d was carried over from the previous rollout with its frames" % t)
        if t == 0 and reset is not True:
            raise ValueError("slot 0 has no previous stack: the first observation of a run is put with reset=True "
                             "(after carry_over() slot 0 already holds the carried stack and the next put is t == 1)")
        if reset is None:
            return self._dones[t - 1]
        if reset is True:
            return self._reset_buf[1]
        if reset is False:
            return None
        r = torch.as_tensor(reset)
        if r.is_cuda and r.dtype == torch.uint8 and r.is_contiguous() and r.device == self.device:
            return r
        return copy_into(self._reset_buf[0], r)

    def _push(self, t, newest, flags):
        """frames[t] <- frames[t-1] shifted by one plane + `newest` (csrc/fstack.hip), on the current stream."""
        # t == 0: every env is reset, the previous stack is read but never used (row T: any slot other than the one being written)
        prev = self.frames[t - 1 if t > 0 else self.T] if self.C > 1 else None
        frame_stack_push(prev, newest, flags, self.frames[t])

    def put_new_frames(self, t, newest, reset=None):
        """ONE new frame per env, uint8 [N,84,84] (device or pinned host) -> pool slot t, whose other planes are slot t-1's shifted by
        one: FrameStackWrapper (warputils.py:112-131) on the device.  reset=None: the envs whose done was recorded for step t-1 start a
        new stack (the natural order is act(t-1) -> env step -> record(t-1, r, d) -> put_new_frames(t, obs)); a tensor [N] overrides the
        recorded dones; reset=True: every env (the first observation of a run, the only legal call for t == 0)."""
        buf = self._single_frame_buffers()
        flags = self._reset_flags(t, reset)
        n = torch.as_tensor(newest)
        direct = (n.is_cuda and n.dtype == torch.uint8 and n.is_contiguous() and n.device == self.device and n.data_ptr() % 16 == 0
                  and tuple(n.shape) == (self.N, 84, 84))
        self._push(t, n if direct else copy_into(buf[2], n), flags)

    def put_new_frames_from_ring(self, t, ring, reset=None):
        """put_new_frames with the frame taken from a pinned ring whose slots hold N * 7056 bytes: hipMemcpyAsync on the copy stream into
        one of two staging buffers (step parity), the compute stream waits for it and runs the push kernel.  Ordered with events only, so
        copy t + 1 still runs under forward t: the DMA of step t waits for the last push kernel that read the same staging
        buffer (step t - 2's); and the FIRST ring-fed put of a rollout, at whatever t (slot 1 after the default carry_over()), orders the
        copy stream behind everything the compute stream holds at that moment (_order_copy_stream)."""
        buf = self._single_frame_buffers()
        flags = self._reset_flags(t, reset)           # before the ring is touched: a refused call consumes no slot
        cur = torch.cuda.current_stream()
        k = t & 1
        self._order_copy_stream()
        if self._pushed[k] is None:
            self._pushed[k] = torch.cuda.Event()
        else:
            self.copy_stream.wait_event(self._pushed[k])
        ring.pop_to(buf[k], stream=self.copy_stream)
        cur.wait_stream(self.copy_stream)
        self._push(t, buf[k], flags)
        self._pushed[k].record(cur)

    # ---- acting ---------------------------------------------------------------------------------
    def act(self, t):
        """Forward + sample on slot t: fills values[t], actions[t], logps[t]; returns actions[t].  A slot below t0 was carried
        over as a complete step (its action has already been sent to the env): nothing is evaluated, the kept action returns."""
        if t < self.t0:
            return self._actions[t]
        self.hp.forward(self.frames[t], seed=self.seed + self.rollouts, stream_id=t, probs=self._probs,
                        value=self.values[t], action=self._actions[t], logp=self._logps[t])
        return self._actions[t]

    def bootstrap(self):
        """The (T+1)-th stored step: its value is the GAE bootstrap (agent.py:130); its action / log-prob land in row T, for a
        host that steps the env with them and keeps the step (carry_over(keep_step=True)).  Returns the action."""
        return self.act(self.T)

    # ---- carry-over + learner batch ---------------------------------------------------------------
    def _carry_observation(self):
        self.frames[0].copy_(self.frames[self.T])

    def batch(self):
        """Zero-copy views in the layout net.learn expects (sample order is irrelevant to the maths)."""
        B = self.N * self.T
        return Experience(states=[self.frames[:self.T].view(B, self.C, 84, 84)], **self._columns(B))


class StateRollout(_RolloutBase):
    """DeviceRollout for the operator-composed nets (nn/generic.py): the observation is a LIST of
    float tensors per env (e.g. robot_nav: laser [1,960], vector [5], pedestrian image [3,48,48]) and
    the action may be continuous.  Same pool layout idea ([time][env] major, everything on the GPU),
    same life cycle: put_states(t, ...) -> act(t) -> record(t, ...) ... bootstrap() -> finish() -> batch().

    normalize_obs (True, or one bool per component; off by default): every put stores the slot as it arrived, adds its RAW rows to the
    pending sums of the component's RunningNorm (the public ``obs_norm[k]``; None for a component left raw), then normalises the slot IN
    PLACE with the affine frozen at the last finish() -- before the first finish() that of a fresh state, or of whatever the host warmed
    ``obs_norm[k]`` with (update / commit / freeze, or load_state_dict).  act() and batch() therefore read the same numbers and stay
    zero-copy.  finish() commits and freezes.  carry_over() moves a slot that is normalised already: it is neither counted nor
    normalised again, so slot 0 of the next rollout carries the statistics of one finish() earlier than slots 1..T (DESIGN.md
    section 6.6).  normalize_returns: see _RolloutBase.

    track_nav_status: record() also takes the env's info words (DeviceNavEnv(emit_info=True).info) into an int32 [T + 1, N] pool and
    finish() feeds rows 0..T-1 to ``nav_status`` (agent.NavStatus), exactly where it feeds ``returns``.

    bootstrap_truncated = S > 0 (off by default): a step that a time limit ended (info bit 4) is no outcome of
    the task, so GAE goes on from the critic's value of the observation the episode ended in instead of from 0.  record() then also
    takes the env's info words and its terminal observations (DeviceNavEnv(emit_final_obs=True).final_obs) and files the truncated
    envs' rows, with one launch and no read-back, into ``final_pools`` ([S, N, *shape] per component: up to S truncations per env and
    rollout; ``slots`` int32 [T + 1, N] names the pool slot of a step, -1 for none).  finish() normalises the pools like the rollout's
    own slots (normalize_obs: the still-frozen affine, nothing is counted), evaluates them with ONE extra forward of the net into
    ``boot`` [S, N] and runs ddrl_gae_bootstrap.  A truncation beyond the S-th of an env in one rollout keeps the terminal treatment
    and is counted (truncations_dropped()); S = env.truncations_per_rollout(T) drops none.  The net must take a batch of S * N."""

    def __init__(self, net, n_envs, state_shapes, horizon=256, gamma=0.99, landa=0.95, device=None, track_returns=False,
                 normalize_obs=None, obs_clip=10.0, normalize_returns=False, reward_clip=10.0, norm_eps=1e-8, track_nav_status=False,
                 bootstrap_truncated=0):
        state_shapes = [tuple(int(d) for d in shape) for shape in state_shapes]
        flags = obs_norm_flags(normalize_obs, len(state_shapes))
        check_knobs(norm_eps, obs_clip)
        self.S = S = int(bootstrap_truncated)
        if S < 0:
            raise ValueError("bootstrap_truncated must be 0 (off) or the pool depth S >= 1, got %d" % S)
        if S > 0 and len(state_shapes) > 4:
            raise ValueError("bootstrap_truncated files at most four observation components, got %d" % len(state_shapes))
        self.net = net
        N, T = int(n_envs), int(horizon)
        super().__init__(net, N, T, gamma, landa, device if device is not None else net.device,
                         action_shape=(T + 1, N, net.n_actions) if getattr(net, "continuous", False) else None,
                         track_returns=track_returns, track_nav_status=track_nav_status, normalize_returns=normalize_returns,
                         reward_clip=reward_clip, norm_eps=norm_eps)
        dev = self.device
        self.states = [torch.empty((T + 1, N) + shape, dtype=torch.float32, device=dev) for shape in state_shapes]
        self.obs_norm = None
        if any(flags):
            self.obs_norm = [RunningNorm(shape, dev, eps=norm_eps, clip=obs_clip) if on else None
                             for on, shape in zip(flags, state_shapes)]
        self.final_pools = self.trunc_count = self.slots = self.boot = None
        if S > 0:
            self.final_pools = [torch.zeros((S, N) + shape, dtype=torch.float32, device=dev) for shape in state_shapes]
            self.trunc_count = torch.zeros(N, dtype=torch.int32, device=dev)
            self.slots = torch.full((T + 1, N), -1, dtype=torch.int32, device=dev)
            self.boot = torch.zeros((S, N), dtype=torch.float32, device=dev)
            if self._infos is None:     # the info pool exists when either this or track_nav_status is on
                self._infos = torch.zeros((T + 1, N), dtype=torch.int32, device=dev)

    def _file_final_obs(self, t, final_obs):
        """record() of a rollout that bootstraps truncated episodes: the rows of the envs whose info word of step t has the truncation
        bit go into slot trunc_count[n] of ``final_pools``, ``slots[t]`` saying which (-1: none, or no room left).  One launch, no
        read-back."""
        file_flagged_rows(self._infos[t], list(zip(final_obs, self.final_pools)), self.trunc_count, self.slots[t])

    def truncations_dropped(self):
        """How many truncations of this rollout found no room in the pools and kept the terminal treatment, clamp(count - S, 0).sum():
        one device-to-host copy, for logs and tests."""
        if self.S == 0:
            return 0
        return int((self.trunc_count - self.S).clamp_(min=0).sum().item())

    def _evaluate_final_pools(self):
        """finish(), in front of the commits: the filed terminal observations become what the net reads -- normalised in place with the
        affine this rollout's own slots were normalised with (still frozen: nothing is counted) -- and one forward writes their values
        into ``boot``.  Pool rows that no slot names are evaluated too and never read."""
        SN = self.S * self.N
        flat = [p.view((SN,) + tuple(p.shape[2:])) for p in self.final_pools]
        for norm, rows in zip(self.obs_norm or (), flat):
            if norm is not None:
                norm.apply(rows, out=rows)
        (_, _), values = self.net(flat, play_mode=True)
        self.boot.view(SN).copy_(values[0][:, 0])

    def _gae(self):
        """_RolloutBase._gae; with bootstrap_truncated the scan is ddrl_gae_bootstrap on the same rewards (the scaled ones under
        normalize_returns: the critic is trained in those units)."""
        if self.S == 0:
            return super()._gae()
        rewards = self.rewards if self.ret_norm is None else self.ret_norm.scale(self.rewards, self.dones)
        gae_bootstrap(self.values, rewards, self.dones, self.slots[:self.T], self.boot, self.gamma, self.landa, self.adv, self.ret)

    def _normalize_slot(self, t, index):
        """Slot t of component `index` holds raw rows: count them, then normalise them in place with the frozen affine."""
        norm = self.obs_norm[index] if self.obs_norm is not None else None
        if norm is not None:
            slot = self.states[index][t]
            norm.update(slot)
            norm.apply(slot, out=slot)

    def put_states(self, t, states):
        """Device or pinned-host tensors, one per observation component -> pool slot t."""
        for k, (pool, s) in enumerate(zip(self.states, states)):
            copy_into(pool[t], torch.as_tensor(s).reshape(pool[t].shape))
            self._normalize_slot(t, k)

    def state_rows(self, t):
        """The pool rows of slot t, one [N, ...] view per component: where a device producer (env/device_nav_env.py) renders the
        observation of slot t, followed by put_states_in_place(t)."""
        return [pool[t] for pool in self.states]

    def put_states_in_place(self, t):
        """Slot t was written through state_rows(t) by a producer on the current stream: nothing is copied.  With normalize_obs the raw
        rows are counted and normalised in place exactly as put_states does; otherwise a no-op."""
        for k in range(len(self.states)):
            self._normalize_slot(t, k)

    def put_state_from_ring(self, t, index, ring):
        """Component `index` of slot t from a pinned ring (raw fp32 bytes), on the copy stream.  The FIRST ring-fed put of a rollout, of
        whatever component and at whatever t (slot 1 after carry_over()), orders the copy stream behind the compute stream
        (_order_copy_stream), with or without normalize_obs: once per rollout, not once per component of the first slot.  Later puts
        land in rows that nothing enqueued since then touches (the in-place normalisation writes the slot it just received)."""
        self._order_copy_stream()
        ring.pop_to(self.states[index][t], stream=self.copy_stream)
        torch.cuda.current_stream().wait_stream(self.copy_stream)
        self._normalize_slot(t, index)

    def act(self, t):
        if t < self.t0:  # carried over as a complete step (DeviceRollout.act)
            return self._actions[t]
        (dist, _), values = self.net([p[t] for p in self.states])
        a = dist.sample()
        self.values[t].copy_(values[0][:, 0])
        self._actions[t].copy_(a)
        self._logps[t].copy_(self.net.actor.log_prob_from_distribution(dist, a))
        return self._actions[t]

    def bootstrap(self, sample=False):
        """Value of the (T+1)-th stored step (agent.py:130).  sample=True also draws its action / log-prob into row T, for a
        host that steps the env with them and keeps the step (carry_over(keep_step=True)); returns that action."""
        if sample:
            return self.act(self.T)
        (_, _), values = self.net([p[self.T] for p in self.states], play_mode=True)
        self.values[self.T].copy_(values[0][:, 0])
        return None

    def _before_gae(self):
        """finish() commits and freezes the observation statistics in component order, in front of the returns' commit; before that,
        while the affine this rollout's slots were normalised with is still frozen, the filed terminal observations are evaluated."""
        if self.S > 0:
            self._evaluate_final_pools()
        for norm in self.obs_norm or ():
            if norm is not None:
                norm.commit()
                norm.freeze()

    def state_dict(self):
        """_RolloutBase.state_dict plus the observation statistics, one entry (or None) per component."""
        sd = super().state_dict()
        sd["obs_norm"] = None if self.obs_norm is None else [None if n is None else n.state_dict() for n in self.obs_norm]
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        saved = sd.get("obs_norm")
        mine = self.obs_norm
        if [n is None for n in saved or ()] != [n is None for n in mine or ()]:
            raise ValueError("normalize_obs differs between the saved rollout and this one")
        for n, s in zip(mine or (), saved or ()):
            if n is not None:
                n.load_state_dict(s)

    def _carry_observation(self):
        """Every component; a slot normalised at its put moves as it is (class docstring).  The pools of terminal observations start
        the next rollout empty."""
        for p in self.states:
            p[0].copy_(p[self.T])
        if self.S > 0:
            self.trunc_count.zero_()
            for p in self.final_pools:
                p.zero_()

    def batch(self):
        B = self.N * self.T
        return Experience(states=[p[:self.T].reshape((B,) + tuple(p.shape[2:])) for p in self.states], **self._columns(B))
