"""PPO minibatch epochs on the Atari fast path: TRAINING_ITER_TIME epochs of PPO_MINIBATCHES optimiser steps each, on shuffled or
contiguous minibatches, with optional advantage normalisation -- what the reference does not have (USTC_lab/nn/ppo.py:77-146 runs
TRAINING_ITER_TIME full-batch steps on raw advantages).

The knobs are read from config_nn with getattr (like PPO_DIAGNOSTICS; the ConfigNN contract does not carry them), by every learner's
constructor through one reader, learner_options() below, which also refuses the Atari-only ones for the operator-composed learners:

  PPO_MINIBATCHES      1       K optimiser steps per epoch; a count, so every rank of a group does the same number of collectives
  PPO_SHUFFLE          False   True: a fresh permutation of this rank's samples every epoch
  NORMALIZE_ADVANTAGE  False   "batch": (adv - mean) / (std + eps) over the whole (global) batch, once per learn call;
                               "minibatch": over every (global) minibatch
  ADV_NORM_EPS         1e-8    the eps above

  FRAMES_IN_PLACE      False   True: no batch or minibatch of frames is staged; the conv1 kernels read the frames where they lie
                               through a frame table (csrc/ftable.hip, ddrl_ppo_iter_indexed).  Same bits.  Not one of the four knobs
                               that choose the step source: the frame source of either reads it (nn/update_loop.py)

  ACT_IN_PLACE         False   True: PlaneRollout.act reads its slot of the single-frame pool where it lies (one ddrl_op_frame_slot launch
                               for the age row and the slot's frame table, then ddrl_forward_indexed) instead of gathering it into a
                               scratch first.  Same bits.  Its own knob: FRAMES_IN_PLACE alone changes nothing about acting

  VALUE_CLIP           None    c > 0: the value loss is clipped around the collecting policy's value, max(e(ret - v), e(ret - v_c)) with
                               v_c = v_old + clamp(v - v_old, -c, c) (the loss kernels' option form, ddrl_ppo_iter_opt); data.values
                               then carries v_old as its row 1
  ENTROPY_BONUS_SPLIT  False   True: with two encoders the actor side differentiates actor_loss - ENTROPY_LOSS_THETA * entropy (the
                               reference differentiates actor_loss alone there, so its entropy coefficient only shows in the logged total)
  LR_ANNEAL_UPDATES    None    N >= 1: before optimiser step u (0-based, steps this net has applied) the three learning rates are
  LR_ANNEAL_FLOOR      0.0     multiplied by max(LR_ANNEAL_FLOOR, 1 - u / N) (ddrl_set_rates);
  CLIP_ANNEAL          False   True: PPO_CLIP as well

PPO.learn runs one loop (nn/update_loop.py run()) over one of two step sources: with all four knobs at their defaults its own single
full-batch step, otherwise steps() below.  Per step, everything on the device and in stream order: shuffle on, one gather of frames
and columns into ONE staging buffer (or, in place, one frame table); off, contiguous views of the columns and of stacked frames
(FramePlanes: the stacks assembled into the same buffer); the moments / affine / normalise operators of csrc/minibatch.hip where
asked for; then the launch and what run() does after it.  split() and epoch_order() are plain CPU functions: a test recomputes
every minibatch from them.
"""
import collections

import torch

from ddrl4nav_amd import ops

DEFAULTS = (1, False, None, 1e-8)
MODES = ("batch", "minibatch")
KNOBS = ("PPO_MINIBATCHES", "PPO_SHUFFLE", "NORMALIZE_ADVANTAGE", "ADV_NORM_EPS")


def minibatch_options(config_nn):
    """(K, shuffle, mode or None, eps) from config_nn; ValueError for K < 1, an unknown mode or a negative eps."""
    k = getattr(config_nn, "PPO_MINIBATCHES", 1)
    if isinstance(k, bool) or int(k) != k or int(k) < 1:
        raise ValueError("PPO_MINIBATCHES must be an integer >= 1, got %r" % (k,))
    mode = getattr(config_nn, "NORMALIZE_ADVANTAGE", False)
    if mode is None or mode is False:
        mode = None
    elif mode not in MODES:
        raise ValueError("NORMALIZE_ADVANTAGE must be False, 'batch' or 'minibatch', got %r" % (mode,))
    eps = float(getattr(config_nn, "ADV_NORM_EPS", 1e-8))
    if not eps >= 0.0:
        raise ValueError("ADV_NORM_EPS must be >= 0, got %r" % (eps,))
    return int(k), bool(getattr(config_nn, "PPO_SHUFFLE", False)), mode, eps


def frames_in_place_option(config_nn):
    """config_nn.FRAMES_IN_PLACE (optional, default False) as a bool; ValueError for anything but True / False."""
    v = getattr(config_nn, "FRAMES_IN_PLACE", False)
    if not isinstance(v, bool):
        raise ValueError("FRAMES_IN_PLACE must be True or False, got %r" % (v,))
    return v


def refuse_frames_in_place(config_nn, who):
    """GenericPPO and GAIL run operator-composed encoders on float states: no conv1 kernel there reads a frame table."""
    if frames_in_place_option(config_nn):
        raise ValueError("FRAMES_IN_PLACE is built for the Atari fast path alone (nn/ppo.py PPO over AtariPreNet), not for %s: unset it"
                         % who)


def act_in_place_option(config_nn):
    """config_nn.ACT_IN_PLACE (optional, default False) as a bool; ValueError for anything but True / False."""
    v = getattr(config_nn, "ACT_IN_PLACE", False)
    if not isinstance(v, bool):
        raise ValueError("ACT_IN_PLACE must be True or False, got %r" % (v,))
    return v


def refuse_act_in_place(config_nn, who):
    """GenericPPO and GAIL act on float states through operator-composed encoders: no acting kernel there reads a frame table."""
    if act_in_place_option(config_nn):
        raise ValueError("ACT_IN_PLACE is built for the Atari fast path alone (nn/ppo.py PPO over AtariPreNet), not for %s: unset it"
                         % who)


def value_clip_option(config_nn):
    """config_nn.VALUE_CLIP (optional): a finite float > 0, or None (None / False = off); ValueError for anything else."""
    v = getattr(config_nn, "VALUE_CLIP", None)
    if v is None or v is False:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < float(v) < float("inf"):
        raise ValueError("VALUE_CLIP must be a finite number > 0, or None / False for off, got %r" % (v,))
    return float(v)


def entropy_split_option(config_nn):
    """config_nn.ENTROPY_BONUS_SPLIT (optional, default False) as a bool; ValueError for anything but True / False."""
    v = getattr(config_nn, "ENTROPY_BONUS_SPLIT", False)
    if not isinstance(v, bool):
        raise ValueError("ENTROPY_BONUS_SPLIT must be True or False, got %r" % (v,))
    return v


def loss_options(config_nn):
    """(value_clip or 0.0, entropy_split): HotPath.loss_options / ops.heads_loss_opt's `options`; ops.NO_LOSS_OPTIONS when both are off."""
    return (value_clip_option(config_nn) or 0.0, entropy_split_option(config_nn))


def anneal_options(config_nn):
    """(N, floor, clip too) from config_nn.LR_ANNEAL_UPDATES / LR_ANNEAL_FLOOR / CLIP_ANNEAL, or None when LR_ANNEAL_UPDATES is None;
    ValueError for N < 1 or not an integer, a floor outside [0, 1], a CLIP_ANNEAL that is no bool, and for a floor or a clip switch set
    without LR_ANNEAL_UPDATES."""
    n = getattr(config_nn, "LR_ANNEAL_UPDATES", None)
    floor = getattr(config_nn, "LR_ANNEAL_FLOOR", 0.0)
    clip = getattr(config_nn, "CLIP_ANNEAL", False)
    if isinstance(floor, bool) or not isinstance(floor, (int, float)) or not 0.0 <= float(floor) <= 1.0:
        raise ValueError("LR_ANNEAL_FLOOR must be a number in [0, 1], got %r" % (floor,))
    if not isinstance(clip, bool):
        raise ValueError("CLIP_ANNEAL must be True or False, got %r" % (clip,))
    if n is None:
        if clip or float(floor) != 0.0:
            raise ValueError("CLIP_ANNEAL / LR_ANNEAL_FLOOR need LR_ANNEAL_UPDATES, the length of the schedule")
        return None
    if isinstance(n, bool) or not isinstance(n, (int, float)) or int(n) != n or int(n) < 1:
        raise ValueError("LR_ANNEAL_UPDATES must be an integer >= 1 or None, got %r" % (n,))
    return int(n), float(floor), clip


def anneal_factor(u, n, floor=0.0):
    """max(floor, 1 - u / n) in double: the factor in front of optimiser step number u (0-based) of a schedule of n steps."""
    return max(float(floor), 1.0 - float(u) / float(n))


def annealed_rates(base, u, n, floor=0.0, clip_too=False):
    """(actor_lr, critic_lr, learning_rate, ppo_clip) of step u from the base four: each product formed in double (Python floats)
    and rounded once to fp32 where HotPath.set_rates hands it over; ppo_clip only with clip_too."""
    s = anneal_factor(u, n, floor)
    a, c, l, p = (float(x) for x in base)
    return a * s, c * s, l * s, (p * s if clip_too else p)


def refuse_loss_options(config_nn, who):
    """The GAIL generator's value loss sums two critics (ppo.py:95-107): neither a clip around ONE old value nor the split backward is
    defined for it."""
    if loss_options(config_nn) != ops.NO_LOSS_OPTIONS:
        raise ValueError("VALUE_CLIP / ENTROPY_BONUS_SPLIT are not built for %s (its value loss sums two critics): unset them" % who)


LearnerOptions = collections.namedtuple("LearnerOptions", "diagnostics target_kl minibatch frames_in_place act_in_place loss_options "
                                                          "lr_anneal base_rates")


def learner_options(config_nn, who=None, two_critics=False):
    """Every optional knob a learner's constructor reads, validated, as a LearnerOptions: PPO_DIAGNOSTICS / TARGET_KL (ops.diag_options;
    ValueError when TARGET_KL meets DEFERRED_LOSS_READBACK), the four minibatch knobs, FRAMES_IN_PLACE, ACT_IN_PLACE, VALUE_CLIP /
    ENTROPY_BONUS_SPLIT, the annealing schedule, and the four base rates the schedule scales.  who (the Atari PPO passes none): a learner
    over operator-composed encoders, named as its messages name it -- it keeps its states as float lists per encoder input, so the
    frame-row collation and the frame tables are refused.  two_critics (NETWORK_TYPE='gail'): the generator's value loss sums two critics
    (ppo.py:95-107), so the diagnostics and the loss options are refused as well."""
    if two_critics and (bool(getattr(config_nn, "PPO_DIAGNOSTICS", False)) or getattr(config_nn, "TARGET_KL", None) is not None):
        raise NotImplementedError("PPO_DIAGNOSTICS / TARGET_KL are not built for %s: the diagnostics head evaluates one critic, the "
                                  "generator's value loss here is the sum over two (ppo.py:95-107), so ExplainedVariance would describe "
                                  "half of what VLoss reports; unset both" % who)
    diagnostics, target_kl = ops.diag_options(config_nn)
    mb = minibatch_options(config_nn)
    if who is not None and mb != DEFAULTS:
        raise ValueError("%s are built for the Atari fast path alone (nn/ppo.py PPO over AtariPreNet), not for %s: unset them"
                         % (" / ".join(KNOBS), who))
    if who is not None:
        refuse_frames_in_place(config_nn, who)
        refuse_act_in_place(config_nn, who)
    if two_critics:
        refuse_loss_options(config_nn, who)
    in_place, loss, anneal = (frames_in_place_option(config_nn), act_in_place_option(config_nn)), loss_options(config_nn), anneal_options(config_nn)
    base_rates = (float(config_nn.ACTOR_LEARNING_RATE), float(config_nn.CRITIC_LEARNING_RATE), float(config_nn.LEARNING_RATE),
                  float(config_nn.PPO_CLIP))
    return LearnerOptions(diagnostics, target_kl, mb, *in_place, loss, anneal, base_rates)


def split(B, K):
    """K consecutive ranges [(lo, hi)] that cover [0, B): range j has B // K + (1 if j < B % K else 0) elements."""
    B, K = int(B), int(K)
    if K < 1 or B < K:
        raise ValueError("PPO_MINIBATCHES = %d does not fit a batch of %d samples: every minibatch needs at least one" % (K, B))
    base, extra = divmod(B, K)
    out, lo = [], 0
    for j in range(K):
        hi = lo + base + (1 if j < extra else 0)
        out.append((lo, hi))
        lo = hi
    return out


_M64 = 2 ** 64 - 1


def _mix(x):
    """splitmix64's finaliser: neighbouring integers give unrelated seeds."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def epoch_order(seed, learn_call, epoch, B):
    """int32 [B] on the host: the permutation of epoch `epoch` of the `learn_call`-th learn() of a net seeded with `seed`.
    torch.randperm on a private CPU generator seeded from the three integers; the global generator is never touched."""
    s = _mix(int(seed) & _M64)
    s = _mix(s ^ (int(learn_call) & _M64))
    s = _mix(s ^ (int(epoch) & _M64))
    g = torch.Generator(device="cpu")
    g.manual_seed(s & (2 ** 63 - 1))
    return torch.randperm(int(B), generator=g, dtype=torch.int64).to(torch.int32)


class Staging:
    """The device buffers of steps(), kept by the net between learn calls: ONE minibatch of frames and columns (stream order
    makes its reuse safe), one scratch advantage column of the whole batch, the three double sums, the affine pair and the moments'
    workspace."""

    def __init__(self, device, frame_shape, cap, B, in_place=False):
        self.cap, self.B, self.frame_shape, self.in_place = int(cap), int(B), tuple(frame_shape), bool(in_place)
        f32 = dict(dtype=torch.float32, device=device)
        # FRAMES_IN_PLACE: no frame buffer at all, one frame table of a minibatch instead (16 bytes per sample)
        self.frames = None if in_place else torch.empty((self.cap,) + self.frame_shape, dtype=torch.uint8, device=device)
        self.tab = torch.empty((self.cap, 4), dtype=torch.int32, device=device) if in_place else None
        self.cols = torch.empty((4, self.cap), **f32)
        self.old_values = None   # [cap], allocated by steps() when the net clips its value loss and shuffles
        self.adv = torch.empty(self.B, **f32)
        self.sums = torch.zeros(3, dtype=torch.float64, device=device)
        self.affine = torch.zeros(2, **f32)
        self.ws = torch.empty(ops.moments_ws_floats(self.B), **f32)

    def fits(self, frame_shape, cap, B, in_place=False):
        return self.frame_shape == tuple(frame_shape) and self.cap >= cap and self.B >= B and self.in_place == bool(in_place)


def advantage_affine(column, n, st, eps, group):
    """st.affine <- (mean, 1 / (std + eps)) of the first n floats of `column` and of the other ranks' columns: the three sums of every
    rank, summed over the group (dist.allreduce_flat: in place on RCCL ranks, through the host where gloo ranks share a GPU), then the
    affine on the device."""
    from ddrl4nav_amd.dist import allreduce_flat
    ops.moments(column, sums=st.sums, ws=st.ws, n=n)
    allreduce_flat(st.sums, group)
    return ops.moments_affine(st.sums, eps, st.affine)


def steps(net, frames, columns, old_values=None):
    """PPO.learn's step source when a knob is set: TRAINING_ITER_TIME epochs of the K minibatches of split(), one Step each.  `frames`:
    uint8 [B, C, 84, 84] or data.FramePlanes; `columns`: actions, old_logps, advs, rets, fp32 [B] on the device; old_values: the fifth
    column of a net with VALUE_CLIP (a view in order, ops.gather_f32 when shuffled), else None."""
    from ddrl4nav_amd.dist import global_batch
    from ddrl4nav_amd.nn.update_loop import Step, frame_source
    K, shuffle, mode, eps = net.minibatch
    actions, old_logps, advs, rets = columns
    B = len(frames)
    ranges = split(B, K)                       # ValueError when K > B
    cap = ranges[0][1] - ranges[0][0]          # the first minibatch is the largest
    net._ensure_capacity(cap)
    group, in_place = net._process_group, net.frames_in_place
    st = net._mb_stage
    if st is None or not st.fits(frames.shape[1:], cap, B, in_place):
        st = net._mb_stage = Staging(net.device, frames.shape[1:], cap, B, in_place)
    if old_values is not None and shuffle and st.old_values is None:
        st.old_values = torch.empty(st.cap, dtype=torch.float32, device=net.device)
    src = frame_source(net._hp, frames, in_place, st.frames, st.tab)
    call = net.learn_calls
    net.learn_calls += 1
    rank = 0
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        rank = torch.distributed.get_rank(group)
    affine = None
    if mode == "batch":
        affine = advantage_affine(advs, B, st, eps, group)
        if not shuffle:                        # nothing is gathered: one pass into the scratch column
            advs = ops.normalize(advs, affine, out=st.adv, n=B)[:B]
            affine = None
    b_globals = {}
    for epoch in range(net.training_iter_time):
        order = epoch_order(net._seed + rank, call, epoch, B).to(net.device) if shuffle else None   # one int32 upload per epoch
        for j, (lo, hi) in enumerate(ranges):
            n = hi - lo
            vo = None
            if shuffle:
                a, o, ad, r = dst = [st.cols[k, :n] for k in range(4)]
                launch = src.gathered(order[lo:hi], n, (actions, old_logps, advs, rets), dst, affine)
                if old_values is not None:
                    vo = ops.gather_f32(old_values, st.old_values, idx=order[lo:hi], n=n)
            else:
                launch = src.contiguous(lo, hi)
                a, o, ad, r = actions[lo:hi], old_logps[lo:hi], advs[lo:hi], rets[lo:hi]
                if old_values is not None:
                    vo = old_values[lo:hi]
            if mode == "minibatch":
                advantage_affine(ad, n, st, eps, group)
                ad = ops.normalize(ad, st.affine, out=ad if shuffle else st.adv, n=n)[:n]   # in place on the staged column
            if j not in b_globals:             # the ranks' j-th sizes: one collective per j, in the first epoch
                b_globals[j] = global_batch(n, group)
            yield Step(launch, a, o, ad, r, b_globals[j], vo)
