"""Thin ctypes wrappers of the operator-level C ABI (include/ddrl.h, ddrl_op_*): generic
convolution, 2x2 max-pool and dense layers on torch-owned device buffers, and the context-free
frame-stack push (ddrl_frame_stack_push).  torch supplies memory
and streams only; the arithmetic runs in csrc/gconv.hip and csrc/glinear.hip.  Used by
ddrl4nav_amd.nn.generic to compose the reference's non-Atari encoders
(USTC_lab/nn/nav_encoder.py, mlp_encoder.py)."""
import functools
import math
from ctypes import byref, c_int32, c_int64, c_void_p

import torch

from . import _lib
from ._lib import ConvDesc, check


def _p(t):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def _st():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t):
    assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), "expected a contiguous fp32 device tensor"
    return t


_U64 = 2 ** 64 - 1
STATS_KEYS = ("ActorLoss", "VLoss", "EntLoss", "PpoTotalLoss", "GradNorm", "ClipCoef")


def stats_dict(row):
    """The statistics tail of a gradient arena (include/ddrl.h DDRL_STATS_FLOATS; a host tensor or array) by name."""
    s = row.numpy() if hasattr(row, "numpy") else row
    return {k: float(s[i]) for i, k in enumerate(STATS_KEYS)}


DIAG_KEYS = ("ApproxKL", "ClipFraction", "ExplainedVariance", "RatioMax")
DIAG_SLOTS = 8   # include/ddrl.h ddrl_op_heads_diag: n, sum k3, clipped, sum ret, sum ret^2, sum e, sum e^2, max ratio


def diag_dict(sums):
    """The diagnostics of a PPO update from the eight sums of ddrl_op_heads_diag / ddrl_ppo_diag (any sequence of 8 numbers on the
    host; plain Python, no GPU): ApproxKL = mean(expm1(x) - x), x = logp - old_logp; ClipFraction = share of samples whose ratio is
    outside 1 +- ppo_clip; ExplainedVariance = 1 - Var(ret - v) / Var(ret), population variances, nan when the returns are constant;
    RatioMax = the largest ratio."""
    s = [float(x) for x in (sums.tolist() if hasattr(sums, "tolist") else sums)]
    n = s[0]
    if n <= 0:
        return {k: math.nan for k in DIAG_KEYS}
    var_ret = s[4] / n - (s[3] / n) ** 2
    var_e = s[6] / n - (s[5] / n) ** 2
    ev = 1.0 - var_e / var_ret if var_ret != 0.0 else math.nan
    return {"ApproxKL": s[1] / n, "ClipFraction": s[2] / n, "ExplainedVariance": ev, "RatioMax": s[7]}


def loss_dict(stats, backup_time, diag=None):
    """The item a learn() generator yields (reference ppo.py:131-146): four losses of stats_dict, PpoBackUpTime, and the diagnostics of
    diag_dict when given."""
    out = {"PpoTotalLoss": stats["PpoTotalLoss"], "ActorLoss": stats["ActorLoss"], "VLoss": stats["VLoss"], "EntLoss": stats["EntLoss"],
           "PpoBackUpTime": backup_time}
    if diag is not None:
        out.update(diag)
    return out


def combine_diag_sums(rows):
    """One global row from the ranks' (or micro-batches') rows, combined in the order given: slots 0-6 summed, slot 7 the largest.
    Every rank that folds the same rows in the same order ends with the same bits."""
    out = [0.0] * DIAG_SLOTS
    for r in rows:
        r = [float(x) for x in (r.tolist() if hasattr(r, "tolist") else r)]
        for k in range(DIAG_SLOTS - 1):
            out[k] += r[k]
        out[7] = r[7] if (r[7] > out[7] or r[7] != r[7]) else out[7]
    return out


def diag_options(config_nn):
    """(diagnostics on, target KL or None) from config_nn.PPO_DIAGNOSTICS / TARGET_KL (both optional, read like
    DEFERRED_LOSS_READBACK).  TARGET_KL implies the diagnostics and needs the host in the loop after every iteration."""
    target = getattr(config_nn, "TARGET_KL", None)
    if target is not None:
        target = float(target)
        if not target > 0.0:
            raise ValueError("TARGET_KL must be a positive number or None, got %r" % (target,))
        if bool(getattr(config_nn, "DEFERRED_LOSS_READBACK", False)):
            raise ValueError("TARGET_KL stops an update from the host after every iteration; DEFERRED_LOSS_READBACK enqueues all "
                             "iterations before the first read-back: set one of the two")
    return bool(getattr(config_nn, "PPO_DIAGNOSTICS", False)) or target is not None, target


def kl_stop(diag, target_kl):
    """The early-stopping rule: the iteration whose loss saw ApproxKL > 1.5 x TARGET_KL is not applied."""
    return target_kl is not None and diag["ApproxKL"] > 1.5 * target_kl


def heads_diag_ws_floats(desc, max_n):
    f = c_int64()
    check(_lib.load().ddrl_op_heads_diag_ws_floats(byref(desc), int(max_n), byref(f)))
    return f.value


def heads_diag(desc, cfg, params, h_actor, h_critic, n, actions, old_logps, rets, sums=None, accumulate=False, logp_out=None,
               value_out=None, ws=None):
    """The eight sums behind diag_dict for n samples of finished 512-wide features (include/ddrl.h ddrl_op_heads_diag; csrc/diag.hip),
    Categorical or Gaussian by `desc`; reads only.  sums: 8 float64 on the device (accumulate: added to, slot 7 raised);
    logp_out / value_out: optional [n] fp32.  Asynchronous on the current stream; returns sums."""
    if sums is None:
        assert not accumulate, "accumulate needs the sums of the earlier calls"
        sums = torch.empty(DIAG_SLOTS, dtype=torch.float64, device=params.device)
    assert sums.dtype == torch.float64 and sums.is_cuda and sums.is_contiguous() and sums.numel() == DIAG_SLOTS
    if ws is None:
        ws = torch.empty(heads_diag_ws_floats(desc, n), dtype=torch.float32, device=params.device)
    check(_lib.load().ddrl_op_heads_diag(byref(desc), byref(cfg), _p(_f32(params)), _p(h_actor), _p(h_critic), int(n), _p(_f32(actions)),
                                         _p(_f32(old_logps)), _p(_f32(rets)), _p(sums), 1 if accumulate else 0, _p(logp_out),
                                         _p(value_out), _p(ws), _st()))
    return sums


def categorical_stats(probs):
    """(probs / sum, log(clamp(.)), entropy) of softmax outputs [n, A], as torch.distributions.Categorical derives them."""
    n, A = probs.shape
    p_hat, logits = torch.empty_like(probs), torch.empty_like(probs)
    ent = torch.empty(n, dtype=torch.float32, device=probs.device)
    check(_lib.load().ddrl_categorical_stats(_p(probs), n, A, _p(p_hat), _p(logits), _p(ent), _st()))
    return p_hat, logits, ent


def categorical_sample(probs, seed, stream_id):
    """Fresh draws (and their log-probs) from Categorical(probs) with the inverse-CDF contract of the acting kernel."""
    n, A = probs.shape
    action = torch.empty(n, dtype=torch.float32, device=probs.device)
    logp = torch.empty(n, dtype=torch.float32, device=probs.device)
    check(_lib.load().ddrl_categorical_sample(_p(probs), n, A, int(seed) & _U64, int(stream_id) & _U64, _p(action), _p(logp), _st()))
    return action, logp


def frame_stack_push(prev, newest, reset, out):
    """FrameStackWrapper.step / .reset on the device (include/ddrl.h, ddrl_frame_stack_push; csrc/fstack.hip): `out` [n,C,84,84] <- `prev`
    [n,C,84,84] shifted by one plane with `newest` [n,84,84] as the last plane; envs whose `reset` byte ([n] uint8, or None) is not zero
    get `newest` in every plane.  All uint8, contiguous, on one device; `prev` may be None when C == 1.  Asynchronous on the current
    stream; returns `out`."""
    n, C = out.shape[0], out.shape[1]
    assert tuple(out.shape) == (n, C, 84, 84) and tuple(newest.shape) == (n, 84, 84), "expected [n,C,84,84] <- [n,84,84]"
    for t in (prev, newest, reset, out):
        assert t is None or (t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and t.device == out.device), \
            "expected contiguous uint8 tensors on one device"
    assert (prev is None and C == 1) or (prev is not None and tuple(prev.shape) == tuple(out.shape)), "prev must have out's shape"
    assert reset is None or tuple(reset.shape) == (n,), "reset must be [n]"
    check(_lib.load().ddrl_frame_stack_push(_p(prev), _p(newest), _p(reset), n, C, _p(out), _st()))
    return out


def heads_bc_ws_floats(n_actions, max_n):
    """Floats of scratch ddrl_op_heads_bc_loss needs for launches of up to max_n samples."""
    f = c_int64()
    check(_lib.load().ddrl_op_heads_bc_ws_floats(int(n_actions), int(max_n), byref(f)))
    return f.value


def heads_bc_loss(w, b, n_actions, h, ld_h, n, labels, n_total, dh, ld_dh, dw, db, stats, ws):
    """Cross-entropy of the Categorical actor's logits against demonstrated actions and its backward through the head layer (include/ddrl.h,
    ddrl_op_heads_bc_loss; csrc/imit.hip): reads h [n][ld_h], w [A][512], b [A], labels [n] (floats); writes dh [n][ld_dh], dw, db and
    stats = (loss share, correct count).  The mean runs over n_total samples.  Asynchronous on the current stream."""
    check(_lib.load().ddrl_op_heads_bc_loss(_p(w), _p(b), int(n_actions), _p(h), int(ld_h), int(n), _p(labels), int(n_total), _p(dh),
                                            int(ld_dh), _p(dw), _p(db), _p(stats), _p(ws), _st()))


def gather_rows_u8(src, idx, dst, labels_src=None, labels_dst=None, n=None):
    """dst[i] = src[idx[i]] for the first n entries of idx (int32, on the device), rows being everything behind the leading axis of the
    contiguous uint8 tensors `src` / `dst`; labels_dst[i] = labels_src[idx[i]] (fp32) in the same launch (include/ddrl.h,
    ddrl_op_gather_rows_u8).  Asynchronous on the current stream; returns dst."""
    n = int(idx.numel() if n is None else n)
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8 and src.is_contiguous() and dst.is_contiguous() and src.is_cuda \
        and dst.is_cuda, "expected contiguous uint8 device tensors"
    assert idx.dtype == torch.int32 and idx.is_cuda and idx.is_contiguous() and idx.numel() >= n, "idx: contiguous int32 on the device"
    row_bytes = src[0].numel()
    assert dst[0].numel() == row_bytes and dst.shape[0] >= n, "dst rows must match src rows"
    for t in (labels_src, labels_dst):
        assert t is None or (t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()), "labels: contiguous fp32 on the device"
    assert labels_src is None or (labels_src.numel() >= src.shape[0] and labels_dst.numel() >= n)
    check(_lib.load().ddrl_op_gather_rows_u8(_p(src), src.shape[0], row_bytes, _p(idx), n, _p(dst), _p(labels_src), _p(labels_dst), _st()))
    return dst


def heads_bc_mse_ws_floats(n_actions, max_n):
    """Floats of scratch ddrl_op_heads_bc_mse needs for launches of up to max_n samples."""
    f = c_int64()
    check(_lib.load().ddrl_op_heads_bc_mse_ws_floats(int(n_actions), int(max_n), byref(f)))
    return f.value


def heads_bc_mse(w, b, n_actions, h, ld_h, n, targets, n_total, dh, ld_dh, dw, db, stats, ws):
    """mean((mu - y)^2) / 2 of a Gaussian actor's mean mu = w h + b against targets fp32 [n][A], over the n_total * A elements of the
    whole batch, and its backward through the head layer (include/ddrl.h ddrl_op_heads_bc_mse; csrc/imit.hip): writes dh [n][ld_dh], dw,
    db and stats = (loss share, sum |mu - y|).  Asynchronous on the current stream."""
    check(_lib.load().ddrl_op_heads_bc_mse(_p(w), _p(b), int(n_actions), _p(h), int(ld_h), int(n), _p(targets), int(n_total), _p(dh),
                                           int(ld_dh), _p(dw), _p(db), _p(stats), _p(ws), _st()))


def gather_rows_f32(src, idx, dst, n=None):
    """dst[i] = src[clamp(idx[i])] for the first n entries of idx (int32, on the device), rows being everything behind the leading axis
    of the contiguous fp32 tensors `src` / `dst`, of any width (include/ddrl.h ddrl_op_gather_rows_f32).  Asynchronous on the current
    stream; returns dst."""
    n = int(idx.numel() if n is None else n)
    _f32(src), _f32(dst)
    assert idx.dtype == torch.int32 and idx.is_cuda and idx.is_contiguous() and idx.numel() >= n, "idx: contiguous int32 on the device"
    row = src[0].numel()
    assert dst[0].numel() == row and dst.shape[0] >= n, "dst rows must match src rows"
    check(_lib.load().ddrl_op_gather_rows_f32(_p(src), src.shape[0], row, _p(idx), n, _p(dst), _st()))
    return dst


def moments_ws_floats(n):
    """Floats of scratch ddrl_op_moments needs for a column of n floats."""
    f = c_int64()
    check(_lib.load().ddrl_op_moments_ws_floats(int(n), byref(f)))
    return f.value


def moments(x, sums=None, accumulate=False, ws=None, n=None):
    """(n, sum x, sum x^2) of the first n floats of x as 3 float64 on the device (include/ddrl.h ddrl_op_moments; csrc/minibatch.hip):
    double sums in a fixed order.  accumulate: added to what `sums` holds.  Asynchronous on the current stream; returns sums."""
    n = int(x.numel() if n is None else n)
    assert x.numel() >= n
    if sums is None:
        assert not accumulate, "accumulate needs the sums of the earlier calls"
        sums = torch.empty(3, dtype=torch.float64, device=x.device)
    assert sums.dtype == torch.float64 and sums.is_cuda and sums.is_contiguous() and sums.numel() == 3
    if ws is None:
        ws = torch.empty(moments_ws_floats(n), dtype=torch.float32, device=x.device)
    check(_lib.load().ddrl_op_moments(_p(_f32(x)), n, _p(sums), 1 if accumulate else 0, _p(_f32(ws)), _st()))
    return sums


def moments_affine(sums, eps, affine=None):
    """(mean, 1 / (std + eps)) as 2 fp32 on the device from the sums of moments(), torch's unbiased std (include/ddrl.h
    ddrl_op_moments_affine).  Nothing visits the host.  Returns affine."""
    if affine is None:
        affine = torch.empty(2, dtype=torch.float32, device=sums.device)
    assert sums.dtype == torch.float64 and sums.is_cuda and sums.is_contiguous() and sums.numel() == 3 and affine.numel() == 2
    check(_lib.load().ddrl_op_moments_affine(_p(sums), float(eps), _p(_f32(affine)), _st()))
    return affine


def normalize(x, affine, out=None, n=None):
    """out[i] = (x[i] - affine[0]) * affine[1] for the first n floats (include/ddrl.h ddrl_op_normalize); out may be x.  Returns out."""
    n = int(x.numel() if n is None else n)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=x.device)
    assert x.numel() >= n and out.numel() >= n and affine.numel() == 2
    check(_lib.load().ddrl_op_normalize(_p(_f32(x)), n, _p(_f32(affine)), _p(_f32(out)), _st()))
    return out


def gather_minibatch(frames, idx, frames_dst, columns=None, columns_dst=None, adv_affine=None, n=None):
    """The collation of one minibatch in one launch (include/ddrl.h ddrl_op_gather_minibatch): frames_dst[i] = frames[idx[i]] for the
    first n entries of idx (int32, on the device) as gather_rows_u8, and columns_dst[k][i] = columns[k][idx[i]] for the four fp32 columns
    (actions, old_logps, advs, rets); entries may be None in both.  adv_affine (2 fp32 on the device): the advantage column is
    normalised on the way, (adv - a[0]) * a[1].  Asynchronous on the current stream; returns frames_dst."""
    n = int(idx.numel() if n is None else n)
    assert frames.dtype == torch.uint8 and frames_dst.dtype == torch.uint8 and frames.is_contiguous() and frames_dst.is_contiguous() \
        and frames.is_cuda and frames_dst.is_cuda, "expected contiguous uint8 device tensors"
    assert idx.dtype == torch.int32 and idx.is_cuda and idx.is_contiguous() and idx.numel() >= n, "idx: contiguous int32 on the device"
    row_bytes = frames[0].numel()
    assert frames_dst[0].numel() == row_bytes and frames_dst.shape[0] >= n, "frames_dst rows must match the frames' rows"
    src, dst = list(columns or (None,) * 4), list(columns_dst or (None,) * 4)
    assert len(src) == 4 and len(dst) == 4, "four columns: actions, old_logps, advs, rets"
    for s, d in zip(src, dst):
        assert (s is None) == (d is None), "a column comes with its destination"
        assert s is None or (_f32(s).numel() >= frames.shape[0] and _f32(d).numel() >= n)
    assert adv_affine is None or (_f32(adv_affine).numel() == 2 and src[2] is not None)
    check(_lib.load().ddrl_op_gather_minibatch(_p(frames), frames.shape[0], row_bytes, _p(idx), n, _p(frames_dst), *[_p(t) for t in src],
                                               *[_p(t) for t in dst], _p(adv_affine), _st()))
    return frames_dst


def gather_f32(src, dst, idx=None, first=0, n=None):
    """One more float column next to the four of the gathers (include/ddrl.h ddrl_op_gather_f32; csrc/minibatch.hip): dst[j] =
    src[idx[j]] (idx int32 on the device), or src[first + j] without an index, for j < n; a sample outside src gives zero.
    Asynchronous on the current stream; returns dst[:n]."""
    n = int((idx.numel() if idx is not None else dst.numel()) if n is None else n)
    assert idx is None or (idx.dtype == torch.int32 and idx.is_cuda and idx.is_contiguous() and idx.numel() >= n), \
        "idx: contiguous int32 on the device"
    assert _f32(dst).numel() >= n
    check(_lib.load().ddrl_op_gather_f32(_p(_f32(src)), src.numel(), _p(idx), int(first), n, _p(dst), _st()))
    return dst[:n]


def _rows2d(x, d):
    """(n, ld) of a fp32 device matrix whose rows hold d used columns: a contiguous tensor of n * d floats, or a 2-D view whose rows
    are ld >= d floats apart."""
    assert x.dtype == torch.float32 and x.is_cuda, "expected a fp32 device tensor"
    if x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == d and x.stride(0) >= d:
        return x.shape[0], x.stride(0)
    assert x.is_contiguous() and x.numel() % d == 0, "expected [n, d] rows (contiguous, or a 2-D view with a row stride)"
    return x.numel() // d, d


@functools.lru_cache(maxsize=256)
def column_moments_ws_floats(n, d):
    """Floats of scratch ddrl_op_column_moments needs for n rows of d columns (a function of the two numbers alone: remembered, a
    rollout asks for the same few shapes at every step)."""
    f = c_int64()
    check(_lib.load().ddrl_op_column_moments_ws_floats(int(n), int(d), byref(f)))
    return f.value


def column_moments(x, d, sums=None, accumulate=False, ws=None):
    """(n, sum x_j, sum x_j^2) of the d columns of x ([n, d] rows, see _rows2d) as 1 + 2 d float64 on the device (include/ddrl.h
    ddrl_op_column_moments; csrc/runnorm.hip): double sums in an order the shape alone fixes.  accumulate: added to what `sums`
    holds.  Asynchronous on the current stream; returns sums."""
    d = int(d)
    n, ld = _rows2d(x, d)
    if sums is None:
        assert not accumulate, "accumulate needs the sums of the earlier calls"
        sums = torch.empty(1 + 2 * d, dtype=torch.float64, device=x.device)
    assert sums.dtype == torch.float64 and sums.is_cuda and sums.is_contiguous() and sums.numel() == 1 + 2 * d
    need = column_moments_ws_floats(n, d)
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=x.device)
    assert _f32(ws).numel() >= need, "ws: column_moments_ws_floats(n, d) floats"
    check(_lib.load().ddrl_op_column_moments(_p(x), n, d, ld, _p(sums), 1 if accumulate else 0, _p(ws), _st()))
    return sums


def running_state(d, device):
    """A fresh running state, float64 [1 + 2 d] = (count 0, mean 0..., var 1...): the defaults of the reference's RunningMeanStd."""
    s = torch.zeros(1 + 2 * int(d), dtype=torch.float64, device=device)
    s[1 + int(d):] = 1.0
    return s


def running_merge(sums, state):
    """RunningMeanStd.update (warputils.py:94-109) of `state` with the pending batch `sums` (include/ddrl.h ddrl_op_running_merge);
    both float64 [1 + 2 d] on the device.  Returns state."""
    d = (sums.numel() - 1) // 2
    for t in (sums, state):
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.numel() == 1 + 2 * d
    check(_lib.load().ddrl_op_running_merge(_p(sums), d, _p(state), _st()))
    return state


def running_affine(state, eps, center=True, affine=None):
    """affine fp32 [2, d] = (shift, scale) of a running state: shift = mean (0 without center), scale = 1 / sqrt(var + eps)
    (include/ddrl.h ddrl_op_running_affine).  Returns affine."""
    d = (state.numel() - 1) // 2
    assert state.dtype == torch.float64 and state.is_cuda and state.is_contiguous() and state.numel() == 1 + 2 * d
    if affine is None:
        affine = torch.empty((2, d), dtype=torch.float32, device=state.device)
    assert _f32(affine).numel() == 2 * d
    check(_lib.load().ddrl_op_running_affine(_p(state), d, float(eps), 1 if center else 0, _p(affine), _st()))
    return affine


def normalize_columns(x, affine, clip, out=None):
    """out[r][j] = clamp((x[r][j] - shift_j) * scale_j, -clip, clip) with affine = (shift, scale) fp32 [2, d] (include/ddrl.h
    ddrl_op_normalize_columns).  x and out: [n, d] rows (see _rows2d); out may be x, and defaults to a new tensor of x's shape.
    Returns out."""
    d = _f32(affine).numel() // 2
    n, ld_x = _rows2d(x, d)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    n_out, ld_out = _rows2d(out, d)
    assert n_out == n, "out must hold the rows of x"
    check(_lib.load().ddrl_op_normalize_columns(_p(x), n, d, ld_x, _p(affine), float(clip), _p(out), ld_out, _st()))
    return out


def discounted_returns(rewards, dones, gamma, carry, trace=None):
    """trace[t] = carry * gamma + rewards[t]; carry = 0 where dones[t] else trace[t], over the T rows of rewards / dones [T, N]
    (include/ddrl.h ddrl_op_discounted_returns); carry fp32 [N] persists between calls.  Returns trace."""
    T, N = rewards.shape
    assert tuple(dones.shape) == (T, N) and dones.dtype == torch.uint8 and dones.is_cuda and dones.is_contiguous()
    if trace is None:
        trace = torch.empty((T, N), dtype=torch.float32, device=rewards.device)
    assert _f32(carry).numel() == N and tuple(_f32(trace).shape) == (T, N)
    check(_lib.load().ddrl_op_discounted_returns(_p(_f32(rewards)), _p(dones), T, N, float(gamma), _p(carry), _p(trace), _st()))
    return trace


ENV_GAMES = {"pong": 0, "catch": 1}   # include/ddrl.h ddrl_op_env_reset / ddrl_op_env_step `game`
ENV_PLANE = 84 * 84


@functools.lru_cache(maxsize=None)
def env_state_ints():
    """The int32 words of one device env's state (include/ddrl.h ddrl_op_env_state_ints; a constant of the library: remembered)."""
    return int(_lib.load().ddrl_op_env_state_ints())


def _env_args(game, state, frame):
    """(game id, n) of a device-env call after the checks both operators share: state int32 [n, env_state_ints()], frame uint8
    [n, 84, 84], contiguous, on one device, the frame's base 16-byte aligned."""
    if game not in ENV_GAMES:
        raise ValueError("game must be one of %s, got %r" % (sorted(ENV_GAMES), game))
    assert state.dtype == torch.int32 and state.is_cuda and state.is_contiguous() and state.dim() == 2 \
        and state.shape[1] == env_state_ints(), "state: contiguous int32 [n, env_state_ints()] on the device"
    n = state.shape[0]
    assert frame.dtype == torch.uint8 and frame.is_cuda and frame.is_contiguous() and tuple(frame.shape) == (n, 84, 84) \
        and frame.device == state.device, "frame: contiguous uint8 [n, 84, 84] on the state's device"
    assert frame.data_ptr() % 16 == 0, "frame: the base must be 16-byte aligned"
    return ENV_GAMES[game], n


def env_reset(game, state, frame, env0=0, seed=0, mask=None):
    """A new first episode for every env of `state`, or for those with a non-zero byte in mask (uint8 [n]), and their first frames
    (include/ddrl.h ddrl_op_env_reset; csrc/denv.hip).  Asynchronous on the current stream; returns frame."""
    g, n = _env_args(game, state, frame)
    assert mask is None or (mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and mask.numel() == n
                            and mask.device == state.device), "mask: contiguous uint8 [n] on the state's device"
    check(_lib.load().ddrl_op_env_reset(g, _p(state), n, int(env0), int(seed) & 0xFFFFFFFF, _p(mask), _p(frame), _st()))
    return frame


def env_step(game, state, actions, frame, reward, done, env0=0, n_actions=6, points=21, max_steps=10000, seed=0):
    """One step of every env (include/ddrl.h ddrl_op_env_step; csrc/denv.hip): actions fp32 [n] -> state (in place), frame uint8
    [n, 84, 84], reward fp32 [n], done uint8 [n].  Asynchronous on the current stream; returns (frame, reward, done)."""
    g, n = _env_args(game, state, frame)
    assert _f32(actions).numel() == n and _f32(reward).numel() == n and actions.device == state.device \
        and reward.device == state.device, "actions / reward: fp32 [n] on the state's device"
    assert done.dtype == torch.uint8 and done.is_cuda and done.is_contiguous() and done.numel() == n \
        and done.device == state.device, "done: contiguous uint8 [n] on the state's device"
    check(_lib.load().ddrl_op_env_step(g, _p(state), n, int(env0), int(n_actions), int(points), int(max_steps), int(seed) & 0xFFFFFFFF,
                                       _p(actions), _p(frame), _p(reward), _p(done), _st()))
    return frame, reward, done


NAV_ENV_SHAPES = [(1, 960), (5,), (3, 48, 48)]   # laser, vector, pedestrian map: what ddrl_op_nav_env_* write per env, fp32
NAV_ENV_HEADINGS = 3840


@functools.lru_cache(maxsize=None)
def nav_env_state_ints():
    """The int32 words of one navigation env's state (include/ddrl.h ddrl_op_nav_env_state_ints; a constant of the library)."""
    return int(_lib.load().ddrl_op_nav_env_state_ints())


def nav_env_trig():
    """The Q14 table the navigation kernels index, as a host tensor int32 [2, 3840] (cos, sin) (include/ddrl.h ddrl_op_nav_env_trig)."""
    out = torch.empty((2, NAV_ENV_HEADINGS), dtype=torch.int32)
    check(_lib.load().ddrl_op_nav_env_trig(c_void_p(out.data_ptr())))
    return out


def _arena_args(state, state_ints, rows_per_state, obs, what="obs"):
    """(n_states, rows) of a navigation-arena call after the checks the nav and the fleet operators share: state int32 [n_states,
    state_ints] and the three components of `obs` fp32 [rows, 1, 960], [rows, 5], [rows, 3, 48, 48] with rows = n_states *
    rows_per_state, contiguous, on one device, laser and image 16-byte aligned."""
    assert state.dtype == torch.int32 and state.is_cuda and state.is_contiguous() and state.dim() == 2 \
        and state.shape[1] == state_ints, "state: contiguous int32 [n, %d] on the device" % state_ints
    rows = state.shape[0] * rows_per_state
    assert len(obs) == 3, "%s: [laser, vector, image]" % what
    for name, t, shape in zip(("laser", "vector", "image"), obs, NAV_ENV_SHAPES):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (rows,) + shape \
            and t.device == state.device, "%s %s: contiguous fp32 %s on the state's device" % (what, name, ("rows",) + shape)
    assert obs[0].data_ptr() % 16 == 0 and obs[2].data_ptr() % 16 == 0, "%s laser / image: the base must be 16-byte aligned" % what
    return state.shape[0], rows


def _arena_mask_ok(mask, state):
    assert mask is None or (mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and mask.numel() == state.shape[0]
                            and mask.device == state.device), "mask: contiguous uint8 [n], a byte a state row, on the state's device"


def _arena_step_ok(state, rows, actions, reward, done):
    assert tuple(_f32(actions).shape) == (rows, 2) and _f32(reward).numel() == rows and actions.device == state.device \
        and reward.device == state.device, "actions fp32 [rows, 2], reward fp32 [rows] on the state's device"
    assert done.dtype == torch.uint8 and done.is_cuda and done.is_contiguous() and done.numel() == rows \
        and done.device == state.device, "done: contiguous uint8 [rows] on the state's device"


def _arena_info_ok(state, rows, info):
    assert info is not None and info.dtype == torch.int32 and info.is_cuda and info.is_contiguous() and tuple(info.shape) == (rows,) \
        and info.device == state.device, "info: contiguous int32 [rows] on the state's device"


def _p3(obs):
    return _p(obs[0]), _p(obs[1]), _p(obs[2])


def nav_env_reset(state, obs, env0=0, seed=0, n_obstacles=10, n_peds=5, mask=None):
    """A new first episode for every env of `state`, or for those with a non-zero byte in mask (uint8 [n]), and their first observations
    obs = [laser, vector, image] (include/ddrl.h ddrl_op_nav_env_reset; csrc/navenv.hip).  Asynchronous on the current stream; returns
    obs."""
    n, _ = _arena_args(state, nav_env_state_ints(), 1, obs)
    _arena_mask_ok(mask, state)
    check(_lib.load().ddrl_op_nav_env_reset(_p(state), n, int(env0), int(seed) & 0xFFFFFFFF, int(n_obstacles), int(n_peds), _p(mask),
                                            *_p3(obs), _st()))
    return obs


def _nav_env_step_args(state, actions, obs, reward, done, env0, seed, n_obstacles, n_peds, max_steps):
    """The checks the three nav_env_step* share, and the arguments all three C entry points take up to `done`."""
    n, _ = _arena_args(state, nav_env_state_ints(), 1, obs)
    _arena_step_ok(state, n, actions, reward, done)
    return (_p(state), n, int(env0), int(seed) & 0xFFFFFFFF, int(n_obstacles), int(n_peds), int(max_steps), _p(actions), *_p3(obs),
            _p(reward), _p(done))


def nav_env_step(state, actions, obs, reward, done, env0=0, seed=0, n_obstacles=10, n_peds=5, max_steps=500):
    """One step of every env (include/ddrl.h ddrl_op_nav_env_step; csrc/navenv.hip): actions fp32 [n, 2] -> state (in place), obs =
    [laser, vector, image], reward fp32 [n], done uint8 [n].  Asynchronous on the current stream; returns (obs, reward, done)."""
    args = _nav_env_step_args(state, actions, obs, reward, done, env0, seed, n_obstacles, n_peds, max_steps)
    check(_lib.load().ddrl_op_nav_env_step(*args, _st()))
    return obs, reward, done


def nav_env_step_info(state, actions, obs, reward, done, info, env0=0, seed=0, n_obstacles=10, n_peds=5, max_steps=500):
    """nav_env_step plus the info word of every env, info int32 [n] (include/ddrl.h ddrl_op_nav_env_step_info): what the step just played
    did -- done, goal, collision kind, truncation, closeness to a pedestrian, the decoded action (nav_info_fields unpacks it).  The other
    outputs are bit-identical to nav_env_step's.  Asynchronous on the current stream; returns (obs, reward, done, info)."""
    args = _nav_env_step_args(state, actions, obs, reward, done, env0, seed, n_obstacles, n_peds, max_steps)
    _arena_info_ok(state, args[1], info)
    check(_lib.load().ddrl_op_nav_env_step_info(*args, _p(info), _st()))
    return obs, reward, done, info


def nav_env_step_final(state, actions, obs, reward, done, info, final_obs, env0=0, seed=0, n_obstacles=10, n_peds=5, max_steps=500):
    """nav_env_step_info plus the terminal observation (include/ddrl.h ddrl_op_nav_env_step_final): for an env
    whose info word has the truncation bit, row i of final_obs = [laser, vector, image] (the observation's shapes) receives the
    observation of the state the episode ended in; no other row of final_obs is written.  The other outputs are bit-identical to
    nav_env_step_info's.  Asynchronous on the current stream; returns (obs, reward, done, info, final_obs)."""
    args = _nav_env_step_args(state, actions, obs, reward, done, env0, seed, n_obstacles, n_peds, max_steps)
    _arena_info_ok(state, args[1], info)
    _arena_args(state, nav_env_state_ints(), 1, final_obs, what="final_obs")
    check(_lib.load().ddrl_op_nav_env_step_final(*args, _p(info), *_p3(final_obs), _st()))
    return obs, reward, done, info, final_obs


NAV_PED_MODELS = ("walk", "avoid")      # include/ddrl.h DDRL_PED_WALK, DDRL_PED_AVOID: the value is the index


def nav_ped_model(ped_model):
    """The DDRL_PED_* value of a pedestrian model given by name ("walk", "avoid") or by value (0, 1); anything else is a ValueError."""
    if isinstance(ped_model, str):
        if ped_model in NAV_PED_MODELS:
            return NAV_PED_MODELS.index(ped_model)
    elif isinstance(ped_model, int) and not isinstance(ped_model, bool) and 0 <= ped_model < len(NAV_PED_MODELS):
        return ped_model
    raise ValueError("ped_model must be one of %r, got %r" % (NAV_PED_MODELS, ped_model))


def _arena_model_tail(state, state_ints, rows_per_state, rows, info, final_obs):
    """The optional outputs of a *_env_step_model call after their checks, as the C entry points take them: info, final_* (nulls for
    what is not given; final_obs needs info)."""
    if info is not None or final_obs is not None:
        _arena_info_ok(state, rows, info)
    if final_obs is None:
        return _p(info), c_void_p(0), c_void_p(0), c_void_p(0)
    _arena_args(state, state_ints, rows_per_state, final_obs, what="final_obs")
    return (_p(info),) + _p3(final_obs)


def nav_env_step_model(state, actions, obs, reward, done, info=None, final_obs=None, ped_model="walk", env0=0, seed=0, n_obstacles=10,
                       n_peds=5, max_steps=500):
    """One step of every env under a pedestrian model (include/ddrl.h ddrl_op_nav_env_step_model): "walk" is
    nav_env_step's rule 1, under "avoid" the pedestrians give way to each other and to the robot (tests/ped_avoid_ref.py).  info int32
    [n] and final_obs = [laser, vector, image] are optional outputs, nav_env_step_info's and nav_env_step_final's (final_obs needs info).
    With "walk" the outputs are bit-identical to the entry point that takes the same outputs.  Asynchronous on the current stream;
    returns (obs, reward, done)."""
    args = _nav_env_step_args(state, actions, obs, reward, done, env0, seed, n_obstacles, n_peds, max_steps)
    tail = _arena_model_tail(state, nav_env_state_ints(), 1, args[1], info, final_obs)
    check(_lib.load().ddrl_op_nav_env_step_model(*args[:7], nav_ped_model(ped_model), *args[7:], *tail, _st()))
    return obs, reward, done


def beta_threshold(beta):
    """The uint32 threshold of DAgger's mixing rate: min(2^32 - 1, floor(beta 2^32)); an env plays the expert where its draw is below."""
    beta = float(beta)
    if not 0.0 <= beta <= 1.0:
        raise ValueError("beta must be in [0, 1], got %r" % (beta,))
    return min(2 ** 32 - 1, int(math.floor(beta * 2.0 ** 32)))


def nav_expert(state, label=None, played=None, policy=None, step=0, threshold=2 ** 32 - 1, env0=0, seed=0, n_obstacles=10, n_peds=5):
    """The scripted expert's action for every env of `state` (include/ddrl.h ddrl_op_nav_expert; csrc/navexpert.hip; the rules are
    tests/nav_expert_ref.py): label fp32 [n, 2] = (v / 32, w / 64) of the arc it prefers; played fp32 [n, 2] = the label where the env's
    draw of `step` is below `threshold` (beta_threshold), policy fp32 [n, 2] elsewhere.  The state is only read.  Asynchronous on the
    current stream; returns (label, played)."""
    ints = nav_env_state_ints()
    assert state.dtype == torch.int32 and state.is_cuda and state.is_contiguous() and state.dim() == 2 and state.shape[1] == ints, \
        "state: contiguous int32 [n, %d] on the device" % ints
    n = state.shape[0]
    for name, t in (("label", label), ("played", played), ("policy", policy)):
        assert t is None or (tuple(_f32(t).shape) == (n, 2) and t.device == state.device), "%s: fp32 [n, 2] on the state's device" % name
    if not 0 <= int(step) < 2 ** 32 or not 0 <= int(threshold) < 2 ** 32:
        raise ValueError("step and threshold must fit 32 bits, got %r and %r" % (step, threshold))
    check(_lib.load().ddrl_op_nav_expert(_p(state), n, int(env0), int(seed) & 0xFFFFFFFF, int(n_obstacles), int(n_peds), _p(policy),
                                         int(step), int(threshold), _p(label), _p(played), _st()))
    return label, played


NAV_INFO_FIELDS = ("done", "goal", "collision", "truncated", "close", "wall_hit", "obstacle_hit", "v", "w")
NAV_COLLISION_STATIC, NAV_COLLISION_PED = 1, 2    # the reference's coding of info["collision"]


def nav_info_fields(info):
    """The fields of info words (a host or device int32 tensor of any shape) as int32 tensors of that shape, by name: done, goal,
    collision (0 none, 1 static, 2 pedestrian), truncated, close, wall_hit, obstacle_hit, and the decoded action v in 0..32 (ticks per
    step) and w in -64..64 (heading steps per step)."""
    w = torch.as_tensor(info)
    assert w.dtype == torch.int32, "info: int32 words"
    bit = lambda k: (w >> k) & 1
    return {"done": bit(0), "goal": bit(1), "collision": (w >> 2) & 3, "truncated": bit(4), "close": bit(5), "wall_hit": bit(6),
            "obstacle_hit": bit(7), "v": (w >> 8) & 63, "w": ((w >> 16) & 255) - 64}


NAV_STATUS_ROWS, NAV_STATUS_RINGS, NAV_STATUS_WINDOW, NAV_STATUS_SUMMARY = 18, 5, 100, 22    # include/ddrl.h DDRL_NAV_STATUS_*


def _nav_status_args(sums, episode_num, rings):
    """N of a navigation-status call after the checks both operators share: sums fp32 [18, N], episode_num int32 [N], rings fp32
    [5, 100, N], contiguous, on one device."""
    assert sums.dtype == torch.float32 and sums.is_cuda and sums.is_contiguous() and sums.dim() == 2 \
        and sums.shape[0] == NAV_STATUS_ROWS, "sums: contiguous fp32 [18, N] on the device"
    N = sums.shape[1]
    assert episode_num.dtype == torch.int32 and episode_num.is_contiguous() and tuple(episode_num.shape) == (N,) \
        and episode_num.device == sums.device, "episode_num: contiguous int32 [N] on the sums' device"
    assert rings.dtype == torch.float32 and rings.is_contiguous() and tuple(rings.shape) == (NAV_STATUS_RINGS, NAV_STATUS_WINDOW, N) \
        and rings.device == sums.device, "rings: contiguous fp32 [5, 100, N] on the sums' device"
    return N


def nav_status_update(info, sums, episode_num, rings):
    """T successive Status.update_nav_status calls over info int32 [T, N] in one launch (include/ddrl.h ddrl_op_nav_status_update;
    csrc/navstat.hip); T == 0 is a no-op.  Asynchronous on the current stream."""
    N = _nav_status_args(sums, episode_num, rings)
    assert info.dtype == torch.int32 and info.is_contiguous() and info.dim() == 2 and info.shape[1] == N \
        and info.device == sums.device, "info: contiguous int32 [T, N] on the sums' device"
    check(_lib.load().ddrl_op_nav_status_update(_p(info) if info.shape[0] else c_void_p(0), int(info.shape[0]), N, _p(sums),
                                                _p(episode_num), _p(rings), _st()))


def nav_status_reduce(sums, episode_num, rings, summary):
    """The (sum, count) pairs group_logger's means are made of, summary float64 [22] (include/ddrl.h ddrl_op_nav_status_reduce): a
    fixed-order sum over the envs.  Asynchronous on the current stream; returns summary."""
    N = _nav_status_args(sums, episode_num, rings)
    assert summary.dtype == torch.float64 and summary.is_contiguous() and tuple(summary.shape) == (NAV_STATUS_SUMMARY,) \
        and summary.device == sums.device, "summary: contiguous float64 [22] on the sums' device"
    check(_lib.load().ddrl_op_nav_status_reduce(_p(sums), _p(episode_num), _p(rings), N, _p(summary), _st()))
    return summary


FLEET_ENV_MAX_ROBOTS = 4          # robots per world of ddrl_op_fleet_env_*; a row is one robot, with the shapes of NAV_ENV_SHAPES


@functools.lru_cache(maxsize=None)
def fleet_env_state_ints():
    """The int32 words of one world's state of the multi-robot navigation env (include/ddrl.h ddrl_op_fleet_env_state_ints)."""
    return int(_lib.load().ddrl_op_fleet_env_state_ints())


def _fleet_env_step_args(state, n_robots, actions, obs, reward, done, info, info_required, world0, seed, n_obstacles, n_peds, max_steps):
    """The arguments both fleet C step entry points take up to `info`, after the checks they share."""
    assert 1 <= int(n_robots) <= FLEET_ENV_MAX_ROBOTS, "n_robots: 1..%d" % FLEET_ENV_MAX_ROBOTS
    n_worlds, rows = _arena_args(state, fleet_env_state_ints(), int(n_robots), obs)
    _arena_step_ok(state, rows, actions, reward, done)
    if info_required or info is not None:
        _arena_info_ok(state, rows, info)
    return (_p(state), n_worlds, int(n_robots), int(world0), int(seed) & 0xFFFFFFFF, int(n_obstacles), int(n_peds), int(max_steps),
            _p(actions), *_p3(obs), _p(reward), _p(done), _p(info))


def fleet_env_reset(state, n_robots, obs, world0=0, seed=0, n_obstacles=10, n_peds=5, mask=None):
    """A new world for every world of `state`, or for those with a non-zero byte in mask (uint8 [n_worlds]), and the first observations
    obs = [laser, vector, image] of their rows (include/ddrl.h ddrl_op_fleet_env_reset; csrc/fleetenv.hip).  Asynchronous on the current
    stream; returns obs."""
    assert 1 <= int(n_robots) <= FLEET_ENV_MAX_ROBOTS, "n_robots: 1..%d" % FLEET_ENV_MAX_ROBOTS
    n_worlds, _ = _arena_args(state, fleet_env_state_ints(), int(n_robots), obs)
    _arena_mask_ok(mask, state)
    check(_lib.load().ddrl_op_fleet_env_reset(_p(state), n_worlds, int(n_robots), int(world0), int(seed) & 0xFFFFFFFF, int(n_obstacles),
                                              int(n_peds), _p(mask), *_p3(obs), _st()))
    return obs


def fleet_env_step(state, n_robots, actions, obs, reward, done, info=None, world0=0, seed=0, n_obstacles=10, n_peds=5, max_steps=500):
    """One step of every world (include/ddrl.h ddrl_op_fleet_env_step; csrc/fleetenv.hip): actions fp32 [rows, 2] -> state (in place),
    obs = [laser, vector, image], reward fp32 [rows], done uint8 [rows] and, when given, info int32 [rows] (nav_info_fields unpacks it;
    collision 3 is another robot); rows = n_worlds * n_robots, row i * n_robots + r is robot r of world i.  Asynchronous on the current
    stream; returns (obs, reward, done)."""
    args = _fleet_env_step_args(state, n_robots, actions, obs, reward, done, info, False, world0, seed, n_obstacles, n_peds, max_steps)
    check(_lib.load().ddrl_op_fleet_env_step(*args, _st()))
    return obs, reward, done


def fleet_env_step_final(state, n_robots, actions, obs, reward, done, info, final_obs, world0=0, seed=0, n_obstacles=10, n_peds=5,
                         max_steps=500):
    """fleet_env_step with info required, plus the terminal observation of every truncated row (include/ddrl.h
    ddrl_op_fleet_env_step_final): what the robot sees with every robot where it is after all moves of the step
    and before any respawn.  Rows without the truncation bit are not written; the other outputs are bit-identical to fleet_env_step's.
    Asynchronous on the current stream; returns (obs, reward, done)."""
    args = _fleet_env_step_args(state, n_robots, actions, obs, reward, done, info, True, world0, seed, n_obstacles, n_peds, max_steps)
    _arena_args(state, fleet_env_state_ints(), int(n_robots), final_obs, what="final_obs")
    check(_lib.load().ddrl_op_fleet_env_step_final(*args, *_p3(final_obs), _st()))
    return obs, reward, done


def fleet_env_step_model(state, n_robots, actions, obs, reward, done, info=None, final_obs=None, ped_model="walk", world0=0, seed=0,
                         n_obstacles=10, n_peds=5, max_steps=500):
    """One step of every world under a pedestrian model (include/ddrl.h ddrl_op_fleet_env_step_model), as
    nav_env_step_model: under "avoid" the pedestrians give way to each other and to every robot.  info and final_obs are optional outputs,
    fleet_env_step's and fleet_env_step_final's (final_obs needs info).  Asynchronous on the current stream; returns (obs, reward, done)."""
    args = _fleet_env_step_args(state, n_robots, actions, obs, reward, done, None, False, world0, seed, n_obstacles, n_peds, max_steps)
    tail = _arena_model_tail(state, fleet_env_state_ints(), int(n_robots), state.shape[0] * int(n_robots), info, final_obs)
    check(_lib.load().ddrl_op_fleet_env_step_model(*args[:8], nav_ped_model(ped_model), *args[8:-1], *tail, _st()))
    return obs, reward, done


NAV_INFO_TRUNCATED = 1 << 4        # the truncation bit of an info word (include/ddrl.h ddrl_op_nav_env_step_info)
FILE_ROWS_MAX_PARTS = 4


def file_flagged_rows(info, parts, count, slot_out, mask=NAV_INFO_TRUNCATED):
    """Files the rows of the envs whose info word has a bit of `mask` into per-env pools (include/ddrl.h ddrl_op_file_flagged_rows;
    csrc/truncate.hip): info int32 [N]; parts = up to four (src fp32 [N, ...], dst fp32 [S, N, ...]) pairs; count int32 [N] (in/out) and
    slot_out int32 [N].  A flagged env n with count[n] < S gets its rows copied to dst[count[n]][n] and slot_out[n] = count[n]; every
    other env slot_out[n] = -1 and no copy; count[n] goes up for every flagged env.  Asynchronous on the current stream, no read-back;
    returns slot_out."""
    assert info.dtype == torch.int32 and info.is_cuda and info.is_contiguous() and info.dim() == 1, "info: contiguous int32 [N] on the device"
    N = info.shape[0]
    for name, t in (("count", count), ("slot_out", slot_out)):
        assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (N,) and t.device == info.device, \
            "%s: contiguous int32 [N] on info's device" % name
    parts = list(parts)
    assert 1 <= len(parts) <= FILE_ROWS_MAX_PARTS, "parts: one to four (src, dst) pairs"
    S = parts[0][1].shape[0]
    widths = []
    for src, dst in parts:
        assert _f32(src).shape[0] == N and src.dim() >= 2 and src.device == info.device, "src: contiguous fp32 [N, ...] on info's device"
        assert _f32(dst).dim() == src.dim() + 1 and tuple(dst.shape) == (S,) + tuple(src.shape) and dst.device == info.device, \
            "dst: contiguous fp32 [S, N, ...] on info's device"
        widths.append(src[0].numel())
    k = len(parts)
    srcs = (c_void_p * k)(*[src.data_ptr() for src, _ in parts])
    dsts = (c_void_p * k)(*[dst.data_ptr() for _, dst in parts])
    check(_lib.load().ddrl_op_file_flagged_rows(_p(info), int(mask), N, int(S), k, srcs, dsts, (c_int32 * k)(*widths), _p(count),
                                                _p(slot_out), _st()))
    return slot_out


def gae_bootstrap(values, rewards, dones, slots, boot, gamma, landa, adv, ret):
    """ddrl_gae with the successor value of flagged steps taken from `boot` (include/ddrl.h ddrl_gae_bootstrap):
    values fp32 [T + 1, N], rewards fp32 [T, N], dones uint8 [T, N], slots int32 [T, N], boot fp32 [S, N]; where slots[t, n] is in
    [0, S) the term (gamma * V_next) * (1 - done) is gamma * boot[slots[t, n], n].  Asynchronous on the current stream; returns
    (adv, ret)."""
    T, N = rewards.shape
    assert tuple(_f32(values).shape) == (T + 1, N) and _f32(rewards).device == values.device, "values fp32 [T + 1, N], rewards fp32 [T, N]"
    assert dones.dtype == torch.uint8 and dones.is_contiguous() and tuple(dones.shape) == (T, N) and dones.device == values.device, \
        "dones: contiguous uint8 [T, N] on the values' device"
    assert slots.dtype == torch.int32 and slots.is_contiguous() and tuple(slots.shape) == (T, N) and slots.device == values.device, \
        "slots: contiguous int32 [T, N] on the values' device"
    assert _f32(boot).dim() == 2 and boot.shape[1] == N and boot.shape[0] >= 1 and boot.device == values.device, "boot: fp32 [S, N]"
    assert tuple(_f32(adv).shape) == (T, N) and tuple(_f32(ret).shape) == (T, N) and adv.device == values.device \
        and ret.device == values.device, "adv / ret: fp32 [T, N] on the values' device"
    check(_lib.load().ddrl_gae_bootstrap(_p(values), _p(rewards), _p(dones), _p(slots), _p(boot), int(boot.shape[0]), int(T), int(N),
                                         float(gamma), float(landa), _p(adv), _p(ret), _st()))
    return adv, ret


NO_LOSS_OPTIONS = (0.0, False)   # (value_clip, entropy_split): both off


def loss_options(value_clip=0.0, entropy_split=False):
    """ddrl_loss_options (include/ddrl.h) from the two update options; value_clip None / False / 0 = off."""
    return _lib.LossOptions(float(value_clip or 0.0), 1 if entropy_split else 0)


def heads_loss_opt(desc, cfg, params, h_actor, h_critic, n, actions, old_logps, advs, rets, options, old_values, b_global, dh_actor,
                   dh_critic, grads, ws):
    """ddrl_op_heads_loss with the update options (include/ddrl.h ddrl_op_heads_loss_opt): `options` = (value_clip, entropy_split),
    old_values [n] fp32 (None unless the clip is on).  Asynchronous on the current stream."""
    o = loss_options(*options)
    check(_lib.load().ddrl_op_heads_loss_opt(byref(desc), byref(cfg), _p(params), _p(h_actor), _p(h_critic), int(n), _p(actions),
                                             _p(old_logps), _p(advs), _p(rets), byref(o), _p(old_values), int(b_global), _p(dh_actor),
                                             _p(dh_critic), _p(grads), _p(ws), _st()))


def frame_age(prev_age, reset, age, channels):
    """The age row of one step of the single-frame pool (include/ddrl.h ddrl_op_frame_age; csrc/fpool.hip): age[i] = 0 where reset[i] is
    not zero, else min(prev_age[i] + 1, channels - 1).  reset None: no env is reset; prev_age None (with a reset array): every env is.
    uint8 [n] on one device.  Asynchronous on the current stream; returns age."""
    for t in (prev_age, reset, age):
        assert t is None or (t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and t.numel() == age.numel()), \
            "expected contiguous uint8 device tensors of one length"
    check(_lib.load().ddrl_op_frame_age(_p(prev_age), _p(reset), age.numel(), int(channels), _p(age), _st()))
    return age


def gather_frame_stacks(planes, age, channels, stacks_dst, idx=None, first=0, n=None, columns=None, columns_dst=None, adv_affine=None,
                        hist=None):
    """Stacks assembled from the single-frame pool in one launch (include/ddrl.h ddrl_op_gather_frame_stacks; csrc/fpool.hip): planes uint8
    [rows, N, 84, 84] with `hist` history rows in front (default channels - 1), age uint8 [rows - hist, N]; stacks_dst[j] [channels, 84,
    84] = the stack of sample idx[j] (int32 on the device), or of sample first + j when idx is None, for j < n.  Columns and adv_affine as
    in gather_minibatch, indexed by the same samples.  Asynchronous on the current stream; returns stacks_dst."""
    C = int(channels)
    hist = C - 1 if hist is None else int(hist)
    for t in (planes, age, stacks_dst):
        assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous(), "expected contiguous uint8 device tensors"
    rows, N = planes.shape[0], planes.shape[1]
    assert tuple(planes.shape[2:]) == (84, 84) and age.numel() >= (rows - hist) * N, "planes [rows,N,84,84], age [rows - hist, N]"
    if idx is not None:
        assert idx.dtype == torch.int32 and idx.is_cuda and idx.is_contiguous(), "idx: contiguous int32 on the device"
        n = int(idx.numel() if n is None else n)
        assert idx.numel() >= n
    n = int(n)
    assert tuple(stacks_dst.shape[1:]) == (C, 84, 84) and stacks_dst.shape[0] >= n, "stacks_dst: [>= n, channels, 84, 84]"
    src, dst = list(columns or (None,) * 4), list(columns_dst or (None,) * 4)
    assert len(src) == 4 and len(dst) == 4, "four columns: actions, old_logps, advs, rets"
    for s, d in zip(src, dst):
        assert (s is None) == (d is None), "a column comes with its destination"
        assert s is None or (_f32(s).numel() >= (rows - hist) * N and _f32(d).numel() >= n)
    assert adv_affine is None or (_f32(adv_affine).numel() == 2 and src[2] is not None)
    check(_lib.load().ddrl_op_gather_frame_stacks(_p(planes), rows, N, hist, _p(age), C, _p(idx), int(first), n, _p(stacks_dst),
                                                  *[_p(t) for t in src], *[_p(t) for t in dst], _p(adv_affine), _st()))
    return stacks_dst


def _table_args(tab, idx, first, n, n_samples, columns, columns_dst, adv_affine):
    """The arguments both frame-table builders share, checked: (tab, idx, first, n, column sources, column destinations)."""
    if idx is not None:
        assert idx.dtype == torch.int32 and idx.is_cuda and idx.is_contiguous(), "idx: contiguous int32 on the device"
        n = int(idx.numel() if n is None else n)
        assert idx.numel() >= n
    n = int(n)
    assert tab.dtype == torch.int32 and tab.is_cuda and tab.is_contiguous() and tab.numel() >= 4 * n, "tab: contiguous int32 [>= n, 4]"
    src, dst = list(columns or (None,) * 4), list(columns_dst or (None,) * 4)
    assert len(src) == 4 and len(dst) == 4, "four columns: actions, old_logps, advs, rets"
    for s, d in zip(src, dst):
        assert (s is None) == (d is None), "a column comes with its destination"
        assert s is None or (_f32(s).numel() >= n_samples and _f32(d).numel() >= n)
    assert adv_affine is None or (_f32(adv_affine).numel() == 2 and src[2] is not None)
    return n, src, dst


def frame_table_planes(planes, age, channels, tab, idx=None, first=0, n=None, columns=None, columns_dst=None, adv_affine=None, hist=None):
    """The frame table of n samples of the single-frame pool (include/ddrl.h ddrl_op_frame_table_planes; csrc/ftable.hip): tab int32
    [>= n, 4], tab[j][c] = index of the plane of `planes` (uint8 [rows, N, 84, 84], `hist` history rows in front, default channels - 1)
    that holds channel c of sample idx[j] (int32 on the device), or of sample first + j when idx is None, by the rule of
    gather_frame_stacks.  Columns and adv_affine as in gather_minibatch.  A sample outside the valid range is CLAMPED to it (the
    gathers return zeros).  No frame is touched.  Asynchronous on the current stream; returns tab."""
    C = int(channels)
    hist = C - 1 if hist is None else int(hist)
    assert age.dtype == torch.uint8 and age.is_cuda and age.is_contiguous(), "age: contiguous uint8 on the device"
    rows, N = planes.shape[0], planes.shape[1]
    assert tuple(planes.shape[2:]) == (84, 84) and age.numel() >= (rows - hist) * N, "planes [rows,N,84,84], age [rows - hist, N]"
    n, src, dst = _table_args(tab, idx, first, n, (rows - hist) * N, columns, columns_dst, adv_affine)
    check(_lib.load().ddrl_op_frame_table_planes(rows, N, hist, _p(age), C, _p(idx), int(first), n, _p(tab), *[_p(t) for t in src],
                                                 *[_p(t) for t in dst], _p(adv_affine), _st()))
    return tab


def frame_table_stacks(frames, tab, idx=None, first=0, n=None, columns=None, columns_dst=None, adv_affine=None):
    """The frame table of n samples of stacked frames uint8 [n_rows, C, 84, 84] (include/ddrl.h ddrl_op_frame_table_stacks):
    tab[j][c] = b * C + c for sample b = idx[j] or first + j, clamped to [0, n_rows); entries c >= C repeat entry C - 1.  Columns and
    adv_affine as in gather_minibatch.  Asynchronous on the current stream; returns tab."""
    assert frames.dim() == 4 and tuple(frames.shape[2:]) == (84, 84), "frames [n_rows, C, 84, 84]"
    n, src, dst = _table_args(tab, idx, first, n, frames.shape[0], columns, columns_dst, adv_affine)
    check(_lib.load().ddrl_op_frame_table_stacks(frames.shape[0], frames.shape[1], _p(idx), int(first), n, _p(tab),
                                                 *[_p(t) for t in src], *[_p(t) for t in dst], _p(adv_affine), _st()))
    return tab


def frame_slot(rows, channels, t, prev_age, reset, age, tab, hist=None):
    """One acting step of the single-frame pool in one launch (include/ddrl.h ddrl_op_frame_slot; csrc/ftable.hip): age (uint8 [N]) as
    frame_age(prev_age, reset, age, channels), and tab (int32 [>= N, 4], 16-byte aligned) as frame_table_planes(first=t * N, n=N) of a
    pool of `rows` plane rows with `hist` history rows in front (default channels - 1), bit for bit.  The table is what
    HotPath.forward_indexed reads slot t through.  Asynchronous on the current stream; returns tab."""
    C = int(channels)
    hist = C - 1 if hist is None else int(hist)
    N = age.numel()
    for x in (prev_age, reset, age):
        assert x is None or (x.dtype == torch.uint8 and x.is_cuda and x.is_contiguous() and x.numel() == N), \
            "expected contiguous uint8 device tensors of one length"
    assert tab.dtype == torch.int32 and tab.is_cuda and tab.is_contiguous() and tab.numel() >= 4 * N, "tab: contiguous int32 [>= N, 4]"
    check(_lib.load().ddrl_op_frame_slot(int(rows), N, hist, C, int(t), _p(prev_age), _p(reset), _p(age), _p(tab), _st()))
    return tab


class Conv:
    """One Conv2d / Conv1d layer (torch weight layout [cout][cin][kh][kw]; Conv1d: h = kh = 1)."""

    def __init__(self, cin, h, w, cout, kh, kw, stride=1, pad=(0, 0), max_n=1, device="cuda"):
        self.lib = _lib.load()
        self.cin, self.h, self.w, self.cout, self.kh, self.kw = cin, h, w, cout, kh, kw
        self.stride, self.pad = stride, tuple(pad)
        self.device = torch.device(device)
        d = self.desc(max_n)
        oh, ow, pf, wf, sf = c_int32(), c_int32(), c_int64(), c_int64(), c_int64()
        check(self.lib.ddrl_op_conv_out_shape(byref(d), byref(oh), byref(ow)))
        check(self.lib.ddrl_op_conv_pack_floats(byref(d), byref(pf)))
        check(self.lib.ddrl_op_conv_ws_floats(byref(d), byref(wf)))
        check(self.lib.ddrl_op_conv_scratch_floats(byref(d), byref(sf)))
        self.oh, self.ow, self.max_n = oh.value, ow.value, max_n
        self.packed = torch.zeros(pf.value, dtype=torch.float32, device=self.device)   # read-only after pack()
        self.ws = torch.empty(wf.value, dtype=torch.float32, device=self.device)
        # per-sample plane scales of a launch that is not handed its scales (fp16-plane layers; max_n floats): one launch per layer
        # object at a time, like `ws`
        self.scratch = torch.empty(sf.value, dtype=torch.float32, device=self.device) if sf.value else None

    def desc(self, n, in_sn=0, out_sn=0):
        return ConvDesc(n, self.cin, self.h, self.w, self.cout, self.kh, self.kw, self.stride, self.pad[0], self.pad[1],
                        in_sn, out_sn)

    def pack(self, weight):
        check(self.lib.ddrl_op_conv_pack(byref(self.desc(1)), _p(_f32(weight)), _p(self.packed), _st()))

    def forward(self, x, bias, relu, out=None, n=None, out_amax=None):
        """out_amax (optional, [n] floats zeroed by the caller): raised to every sample's largest |output| (include/ddrl.h,
        "per-sample magnitudes")."""
        n = x.shape[0] if n is None else n
        assert n <= self.max_n, "batch larger than the layer's scratch was sized for"
        if out is None:
            out = torch.empty((n, self.cout, self.oh, self.ow), dtype=torch.float32, device=x.device)
        check(self.lib.ddrl_op_conv_forward(byref(self.desc(n)), _p(_f32(x)), _p(self.packed), _p(_f32(bias)),
                                            1 if relu else 0, _p(out), _p(self.scratch), _p(out_amax), _st()))
        return out

    def has_forward_pool(self):
        """True when the layer's kernels take ReLU + max_pool2d(2) into their epilogue (include/ddrl.h ddrl_op_conv_forward_pool)."""
        return bool(self.lib.ddrl_op_conv_has_forward_pool(byref(self.desc(1))))

    def pooled_uses_scales(self):
        """True when the pooled operators of this layer read per-sample magnitudes (in_amax / dpool_amax; sample_amax below)."""
        return bool(self.lib.ddrl_op_conv_pooled_uses_scales(byref(self.desc(1))))

    def forward_pool(self, x, bias, pooled, code, n=None, in_amax=None, out_amax=None):
        """max_pool2d(relu(conv(x)), 2) in one launch: pooled [n][cout][oh/2][ow/2] + one decision byte per window.
        in_amax: the samples' largest |x| (from x's producer or sample_amax; None = own pre-pass); out_amax: raised to the samples'
        largest pooled value (zeroed by the caller)."""
        n = x.shape[0] if n is None else n
        assert n <= self.max_n, "batch larger than the layer's scratch was sized for"
        check(self.lib.ddrl_op_conv_forward_pool(byref(self.desc(n)), _p(_f32(x)), _p(self.packed), _p(_f32(bias)), _p(pooled),
                                                 _p(code), _p(in_amax), _p(self.scratch), _p(out_amax), _st()))
        return pooled

    def dgrad_pooled(self, dpool, code, din=None, n=None, dpool_amax=None, din_amax=None):
        """Data gradient of a forward_pool layer from d(pooled) + decision bytes (no full-resolution gradient in between).
        din_amax: raised to the samples' largest |din| (zeroed by the caller)."""
        n = dpool.shape[0] if n is None else n
        assert n <= self.max_n, "batch larger than the layer's scratch was sized for"
        if din is None:
            din = torch.empty((n, self.cin, self.h, self.w), dtype=torch.float32, device=dpool.device)
        check(self.lib.ddrl_op_conv_dgrad_pooled(byref(self.desc(n)), _p(_f32(dpool)), _p(code), _p(self.packed), _p(din),
                                                 _p(dpool_amax), _p(self.scratch), _p(din_amax), _st()))
        return din

    def wgrad_pooled(self, x, dpool, code, dw, db, n=None, in_amax=None, dpool_amax=None):
        n = x.shape[0] if n is None else n
        assert n <= self.max_n, "batch larger than the split-K scratch was sized for"
        check(self.lib.ddrl_op_conv_wgrad_pooled(byref(self.desc(n)), _p(_f32(x)), _p(_f32(dpool)), _p(code), _p(self.packed),
                                                 _p(self.ws), _p(dw), _p(db), _p(in_amax), _p(dpool_amax), _st()))

    def dgrad(self, dz, din=None, n=None):
        n = dz.shape[0] if n is None else n
        assert n <= self.max_n, "batch larger than the layer's scratch was sized for"
        if din is None:
            din = torch.empty((n, self.cin, self.h, self.w), dtype=torch.float32, device=dz.device)
        check(self.lib.ddrl_op_conv_dgrad(byref(self.desc(n)), _p(_f32(dz)), _p(self.packed), _p(din), _p(self.scratch), _st()))
        return din

    def wgrad(self, x, dz, dw, db, n=None):
        n = x.shape[0] if n is None else n
        assert n <= self.max_n, "batch larger than the split-K scratch was sized for"
        check(self.lib.ddrl_op_conv_wgrad(byref(self.desc(n)), _p(_f32(x)), _p(_f32(dz)), _p(self.packed), _p(self.ws),
                                          _p(dw), _p(db), _st()))


def sample_amax(x, n, out):
    """Largest magnitude of every sample of x[:n] (dense samples): the pre-pass for tensors whose producer leaves none (include/ddrl.h)."""
    elems = x[0].numel()
    check(_lib.load().ddrl_op_sample_amax(_p(_f32(x)), elems, elems, n, _p(out), _st()))
    return out


def maxpool2(x, out=None):
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    check(_lib.load().ddrl_op_maxpool2_forward(_p(_f32(x)), n * c, h, w, _p(out), _st()))
    return out


def maxpool2_relu_backward(a, dpool, dz=None):
    n, c, h, w = a.shape
    if dz is None:
        dz = torch.empty_like(a)
    check(_lib.load().ddrl_op_maxpool2_relu_backward(_p(_f32(a)), _p(_f32(dpool)), n * c, h, w, _p(dz), _st()))
    return dz


def maxpool2_idx(x, out=None, code=None):
    """max_pool2d(x, 2) that also leaves one decision byte per window for maxpool2_backward_idx (include/ddrl.h)."""
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    if code is None:
        code = torch.empty((n, c, h // 2, w // 2), dtype=torch.uint8, device=x.device)
    check(_lib.load().ddrl_op_maxpool2_forward_idx(_p(_f32(x)), n * c, h, w, _p(out), _p(code), _st()))
    return out, code


def maxpool2_backward_idx(dpool, code, h, w, dz=None):
    n, c = dpool.shape[:2]
    if dz is None:
        dz = torch.empty((n, c, h, w), dtype=torch.float32, device=dpool.device)
    check(_lib.load().ddrl_op_maxpool2_backward_idx(_p(_f32(dpool)), _p(code), n * c, h, w, _p(dz), _st()))
    return dz


class Linear:
    """One nn.Linear(K, N) (+ReLU) layer; weight [N][K]."""

    def __init__(self, K, N, max_n=1, device="cuda"):
        self.lib = _lib.load()
        self.K, self.N, self.max_n = K, N, max_n
        self.device = torch.device(device)
        a, b, wf = c_int64(), c_int64(), c_int64()
        check(self.lib.ddrl_op_linear_pack_floats(K, N, byref(a), byref(b)))
        check(self.lib.ddrl_op_linear_ws_floats(max_n, K, N, byref(wf)))
        self.wt = torch.zeros(a.value, dtype=torch.float32, device=self.device)
        self.wn = torch.zeros(b.value, dtype=torch.float32, device=self.device)
        self.ws = torch.empty(wf.value, dtype=torch.float32, device=self.device)

    def pack(self, weight):
        check(self.lib.ddrl_op_linear_pack(_p(_f32(weight)), self.K, self.N, _p(self.wt), _p(self.wn), _st()))

    def uses_planes(self, n):
        """True when a launch of n rows runs on the fp16 plane kernels (and therefore reads per-row scales)."""
        return bool(self.lib.ddrl_op_linear_uses_planes(n, self.K, self.N))

    def row_amax(self, x, ld, width, n, out, accumulate=False):
        """Largest magnitude of every row of x[:n] (one pass; hand it to the operators that read the same tensor)."""
        check(self.lib.ddrl_op_row_amax(_p(x), ld, width, n, _p(out), 1 if accumulate else 0, _st()))
        return out

    def forward(self, x, ld_in, bias, relu, out, ld_out, n, in_amax=None):
        assert n <= self.max_n
        check(self.lib.ddrl_op_linear_forward(_p(x), ld_in, _p(self.wt), _p(_f32(bias)), 1 if relu else 0, _p(out), ld_out,
                                              n, self.K, self.N, _p(self.ws), _p(in_amax), _st()))
        return out

    def dgrad(self, dout, ld_dout, mask_src, ld_mask, din, ld_din, n, dout_amax=None, din_amax=None, amax_cols=None):
        """din_amax ([n] floats zeroed by the caller): raised to every row's largest |din| over the columns amax_cols = (lo, hi)
        (default: all K)."""
        assert n <= self.max_n
        lo, hi = amax_cols if amax_cols is not None else (0, 0)
        check(self.lib.ddrl_op_linear_dgrad(_p(dout), ld_dout, _p(self.wn), _p(mask_src), ld_mask, _p(din), ld_din, n,
                                            self.K, self.N, _p(self.ws), _p(dout_amax), _p(din_amax), lo, hi, _st()))
        return din

    def wgrad(self, x, ld_in, dout, ld_dout, dw, db, n, in_amax=None, dout_amax=None):
        assert n <= self.max_n
        check(self.lib.ddrl_op_linear_wgrad(_p(x), ld_in, _p(dout), ld_dout, _p(self.ws), _p(dw), _p(db), n, self.K,
                                            self.N, _p(in_amax), _p(dout_amax), _st()))
