"""FramePlanes: the states of a learner batch whose Atari frames are stored ONCE (agent/plane_rollout.py PlaneRollout.batch()).

  planes uint8 [H + T + 1, N, 84, 84]   H = C - 1 history rows; row H + t is the one frame that arrived for step t
  age    uint8 [T + 1, N]               steps since env i's stack was last reset, saturated at C - 1

Sample b = t * N + i (the order of DeviceRollout.batch()) is the stack whose channel c is pool row H + t - min(C - 1 - c, age[b], H + t)
of env i; csrc/fpool.hip (ddrl_op_gather_frame_stacks) assembles it where it is read.  Only the Atari fast path (nn/ppo.py PPO) reads
this form, through the one frame source over it (nn/update_loop.py PlaneFrames): a minibatch step gathers its stacks from it, the
full-batch step materialises the batch once per learn call -- or, with config_nn.FRAMES_IN_PLACE, both read the planes where they lie
through a frame table (table(); csrc/ftable.hip)."""
import torch

from ddrl4nav_amd import ops


class FramePlanes:
    def __init__(self, planes, age, T, N, C):
        self.T, self.N, self.C = int(T), int(N), int(C)
        H = self.C - 1
        if not 1 <= self.C <= 4:
            raise ValueError("1 to 4 stacked frames, got %d" % self.C)
        if tuple(planes.shape) != (H + self.T + 1, self.N, 84, 84) or tuple(age.shape) != (self.T + 1, self.N):
            raise ValueError("planes must be [C - 1 + T + 1, N, 84, 84] and age [T + 1, N], got %s and %s"
                             % (tuple(planes.shape), tuple(age.shape)))
        if planes.dtype != torch.uint8 or age.dtype != torch.uint8:
            raise ValueError("planes and age are uint8")
        self.planes, self.age = planes, age

    def __len__(self):
        return self.T * self.N

    @property
    def shape(self):
        """The shape of the batch once materialised."""
        return (len(self), self.C, 84, 84)

    def gather(self, out, idx=None, first=0, n=None, columns=None, columns_dst=None, adv_affine=None):
        """out[j] = the stack of sample idx[j] (int32 on the device), or of sample first + j, for j < n, with the columns of
        ops.gather_minibatch riding along.  Samples are valid in [0, len(self)): row T, the bootstrap step, is not part of the batch."""
        H = self.C - 1
        return ops.gather_frame_stacks(self.planes[:H + self.T], self.age[:self.T], self.C, out, idx=idx, first=first, n=n,
                                       columns=columns, columns_dst=columns_dst, adv_affine=adv_affine)

    @property
    def pool(self):
        """The planes a table of table() counts from: the rows of the batch (history included, the bootstrap row not)."""
        return self.planes[:self.C - 1 + self.T]

    def table(self, tab=None, idx=None, first=0, n=None, columns=None, columns_dst=None, adv_affine=None):
        """tab int32 [>= n, 4]: where the stack of sample idx[j] (or first + j) lies in `pool`, for HotPath.ppo_iter_indexed, with the
        columns of ops.gather_minibatch riding along (ops.frame_table_planes).  No frame is moved.  Returns tab."""
        if tab is None:
            tab = torch.empty((int(idx.numel() if n is None else n), 4), dtype=torch.int32, device=self.planes.device)
        return ops.frame_table_planes(self.pool, self.age[:self.T], self.C, tab, idx=idx, first=first, n=n, columns=columns,
                                      columns_dst=columns_dst, adv_affine=adv_affine)

    def stacks(self, lo, hi, out=None):
        """Samples lo..hi-1 materialised as uint8 [hi - lo, C, 84, 84] (into the front of `out` when given); returns that view."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= len(self):
            raise ValueError("samples %d..%d of a batch of %d" % (lo, hi, len(self)))
        if out is None:
            out = torch.empty((hi - lo, self.C, 84, 84), dtype=torch.uint8, device=self.planes.device)
        return self.gather(out, first=lo, n=hi - lo)[:hi - lo]


def planes_of(states):
    """The FramePlanes of an Experience's states, or None."""
    s = states[0] if isinstance(states, (list, tuple)) and len(states) else states
    return s if isinstance(s, FramePlanes) else None


def refuse_frame_planes(states, who):
    """The operator-composed nets keep their states as float tensors per encoder input: nothing there assembles stacks from planes."""
    if planes_of(states) is not None:
        raise TypeError("FramePlanes states (PlaneRollout.batch()) are read by the Atari fast path alone (nn/ppo.py PPO over AtariPreNet), "
                        "not by %s: use DeviceRollout, or materialise the batch with FramePlanes.stacks()" % who)
