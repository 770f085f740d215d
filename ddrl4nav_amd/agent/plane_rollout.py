"""PlaneRollout: DeviceRollout (agent/rollout.py) with every Atari frame stored ONCE.

DeviceRollout keeps whole stacks, uint8 [T+1, N, C, 84, 84]: with single-frame ingest (put_new_frames*) every frame that arrives is
written C times.  Here the pool is

  planes uint8 [H + T + 1, N, 84, 84]   H = C - 1 history rows; row H + t is the one frame that arrived for step t
  age    uint8 [T + 1, N]               steps since env i's stack was last reset, saturated at C - 1 (csrc/fpool.hip ddrl_op_frame_age)

a quarter of the bytes at C = 4 (0.47 GB against 1.86 GB at 256 envs x 256 steps), and a stack is assembled where it is read
(ddrl_op_gather_frame_stacks): act(t) gathers slot t into one [N, C, 84, 84] scratch, the learner gathers its minibatches from
batch().states[0], a data.FramePlanes.  Same life cycle and the same methods as DeviceRollout except the whole-stack puts; the same
actions, log-probs, values and updates bit for bit (tests/test_plane_pool_gpu.py).  The constructor, record(), finish() and carry_over()
ARE DeviceRollout's (agent/rollout.py _RolloutBase): this class supplies the observation pool (_alloc_observation), how it is carried
over (_carry_observation), its puts, act() and the `states` of batch().  The ring-fed put needs no staging buffers and no per-parity
events: the DMA lands in the pool's plane row itself; its copy stream is ordered by the one rule, _order_copy_stream.

act_in_place (None: the net's config_nn.ACT_IN_PLACE, nn/minibatch.py; off by default): act(t) gathers nothing.  The put's age launch is
ops.frame_slot, which also writes the slot's frame table (int32 [N, 4], 16 bytes per env instead of the N * C * 7056 of the scratch), and
act(t) is HotPath.forward_indexed on the pool through that table: the same four launches per step as DeviceRollout, the same bits as the
gathered path (tests/test_act_in_place_gpu.py).  The scratch is then allocated only when stacks() is asked for without `out`."""
import torch

from ddrl4nav_amd import ops
from ddrl4nav_amd.agent.rollout import DeviceRollout
from ddrl4nav_amd.data import Experience, FramePlanes
from ddrl4nav_amd.utils.staging import copy_into


class PlaneRollout(DeviceRollout):
    def __init__(self, net, n_envs, horizon=256, channels=4, gamma=0.99, landa=0.95, device=None, seed=0, track_returns=False,
                 act_in_place=None, normalize_returns=False, reward_clip=10.0, norm_eps=1e-8):
        C, T = int(channels), int(horizon)
        if not 1 <= C <= 4:                # both refused before anything is allocated
            raise ValueError("1 to 4 stacked frames, got %d" % C)
        if T < C:
            raise ValueError("horizon %d < channels %d: carry_over() moves pool rows T..T+C-1 to rows 0..C-1, which would overlap" % (T, C))
        self.H = C - 1
        self.act_in_place = bool(getattr(net, "act_in_place", False) if act_in_place is None else act_in_place)
        super().__init__(net, n_envs, horizon=T, channels=C, gamma=gamma, landa=landa, device=device, seed=seed,
                         track_returns=track_returns, normalize_returns=normalize_returns, reward_clip=reward_clip, norm_eps=norm_eps)

    def _alloc_observation(self):
        """DeviceRollout's constructor with `frames` replaced by planes + age, and what acting on them needs."""
        N, T, dev = self.N, self.T, self.device
        self.planes = torch.empty((self.H + T + 1, N, 84, 84), dtype=torch.uint8, device=dev)
        self.age = torch.zeros((T + 1, N), dtype=torch.uint8, device=dev)
        # the slot act(t) reads: gathered into _stack, or in place through _slot_tab, the frame table of slot _slot_t (-1: of none)
        self._stack = None if self.act_in_place else torch.empty((N, self.C, 84, 84), dtype=torch.uint8, device=dev)
        self._slot_tab = torch.empty((N, 4), dtype=torch.int32, device=dev) if self.act_in_place else None
        self._slot_t = -1
        self._reset_buf = torch.ones((2, N), dtype=torch.uint8, device=dev)   # _reset_flags: 0 a caller's flags, 1 all ones

    # ---- ingest ---------------------------------------------------------------------------------
    def put_frames(self, t, frames):
        raise ValueError("PlaneRollout stores single frames (put_new_frames*): whole stacks go to DeviceRollout")

    def put_frames_from_ring(self, t, ring):
        raise ValueError("PlaneRollout stores single frames (put_new_frames_from_ring): whole stacks go to DeviceRollout")

    def _age(self, t, flags):
        """age[t] from age[t-1] and the reset flags (t == 0: every env is reset, _reset_flags admits nothing else)."""
        prev = self.age[t - 1] if t > 0 else None
        if self.act_in_place:   # the same launch also tables slot t for act(t)
            ops.frame_slot(self.planes.shape[0], self.C, t, prev, flags, self.age[t], self._slot_tab)
            self._slot_t = t
        else:
            ops.frame_age(prev, flags, self.age[t], self.C)

    def put_new_frames(self, t, newest, reset=None):
        """ONE new frame per env, uint8 [N,84,84] (device or pinned host) -> pool row H + t; `reset` as DeviceRollout.put_new_frames.
        `newest` may be new_frame_row(t) itself, already filled: then only the age / slot launch runs."""
        flags = self._reset_flags(t, reset)
        row = self.planes[self.H + t]
        n = torch.as_tensor(newest)
        # a producer on the device (env/device_env.py) may have rendered into new_frame_row(t) itself: nothing is left to copy
        if not (n.is_cuda and n.data_ptr() == row.data_ptr() and n.shape == row.shape and n.dtype == row.dtype and n.is_contiguous()):
            copy_into(row, n)
        self._age(t, flags)

    def new_frame_row(self, t):
        """Pool row H + t, uint8 [N, 84, 84] (16-byte aligned): where put_new_frames(t, ...) stores the frame.  A device producer writes
        it there and passes this very tensor to put_new_frames, which then copies nothing."""
        return self.planes[self.H + t]

    def put_new_frames_from_ring(self, t, ring, reset=None):
        """put_new_frames with the frame taken from a pinned ring whose slots hold N * 7056 bytes: hipMemcpyAsync on the copy stream straight
        into pool row H + t, which nothing enqueued earlier in this rollout touches; the compute stream waits for it.  The FIRST such put
        of a rollout, at whatever t, orders the copy stream behind the compute stream (_order_copy_stream: the previous update and
        carry_over() still read and write the pool); later puts do not wait again, so copy t + 1 runs under forward t."""
        flags = self._reset_flags(t, reset)           # before the ring is touched: a refused call consumes no slot
        self._order_copy_stream()
        ring.pop_to(self.planes[self.H + t], stream=self.copy_stream)
        torch.cuda.current_stream().wait_stream(self.copy_stream)
        self._age(t, flags)

    # ---- acting ---------------------------------------------------------------------------------
    def stacks(self, t, out=None):
        """Slot t (0..T) assembled as uint8 [N, C, 84, 84], into `out` or the scratch act() reads (acting in place: allocated here, at
        the first call without `out`)."""
        if out is None:
            if self._stack is None:
                self._stack = torch.empty((self.N, self.C, 84, 84), dtype=torch.uint8, device=self.device)
            out = self._stack
        return ops.gather_frame_stacks(self.planes, self.age, self.C, out, first=t * self.N, n=self.N)

    def act(self, t):
        """DeviceRollout.act on the gathered slot, or (act_in_place) on the pool through the slot's frame table."""
        if t < self.t0:
            return self._actions[t]
        if self.act_in_place:
            if self._slot_t != t:   # no put tabled this slot (act(0) after carry_over(), a slot acted on again): table it from age[t]
                ops.frame_table_planes(self.planes, self.age, self.C, self._slot_tab, first=t * self.N, n=self.N)
                self._slot_t = t
            self.hp.forward_indexed(self.planes, self._slot_tab, self.N, seed=self.seed + self.rollouts, stream_id=t, probs=self._probs,
                                    value=self.values[t], action=self._actions[t], logp=self._logps[t])
            return self._actions[t]
        self.hp.forward(self.stacks(t), seed=self.seed + self.rollouts, stream_id=t, probs=self._probs,
                        value=self.values[t], action=self._actions[t], logp=self._logps[t])
        return self._actions[t]

    # ---- carry-over + learner batch ---------------------------------------------------------------
    def _carry_observation(self):
        """carry_over(): the last stored step's frame WITH its history (pool rows T..T+H -> 0..H, age[T] -> age[0])."""
        T, H = self.T, self.H
        self.planes[:H + 1].copy_(self.planes[T:T + H + 1])
        self.age[0].copy_(self.age[T])
        self._slot_t = -1          # slot 0 now holds another step's frames: whatever the table describes is stale

    def batch(self):
        """DeviceRollout.batch with the states as FramePlanes over the pool (zero-copy)."""
        return Experience(states=[FramePlanes(self.planes, self.age, self.T, self.N, self.C)], **self._columns(self.N * self.T))
