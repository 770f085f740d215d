"""Direct tests of the small operators behind the PPO iteration: the loss block of both head families on every branch of
the dual-clip surrogate, acting, the clip + Adam / RMSprop steps element by element, and the remaining helpers
(value head, WGAN terms, column sums, ReLU mask, accumulate, row / sample magnitudes) -- each through the C ABI
(include/ddrl.h) against a plain float64 restatement (tests/heads_ref.py).

Yardstick of the loss block and the optimiser steps: torch's own fp32 CPU evaluation of the same expressions on the same
inputs, both measured against float64 -- err_kernel <= 1.25 x err_torch32 (tests/parity_util.py VS_TORCH_LIMIT), the raw
ratio of the two mean errors, logged through P.MARGINS.  A yardstick below the rounding floor (heads_ref.FLOOR) or a mean
over fewer than 64 draws has no ratio (judge() says why); those, the narrow sums (bias / log_std gradients, loss shares)
and the operators of section 4 take the operator tolerance of tests/test_ops_gpu.py, 2e-5 * max|want| + 1e-7 ("same
products, other summation order").

Measured on an MI355X (largest raw ratio per quantity over the cases that are judged): categorical dh_actor 1.15,
dh_critic 0.70, dh_shared 0.87, actor_w 1.07, act logp 1.05; Gaussian dh_actor 0.89, dh_critic 0.73, dh_shared 0.81,
actor_w 1.01; critic_w 0.62; Adam update 1.21, v 1.00, m 0.41; RMSprop square_avg 1.03.  In dh_critic and dh_shared the
one row in seven whose return equals the value to rounding is held to the operator tolerance only (check_heads_loss);
at n <= 64 every feature gradient is (fewer than 64 judged rows).  Printed, not judged (too few draws): categorical dh_actor 1.43 at n = 64
(33 rows with a gradient), act logp 1.58 at n = 3, act dist 1.47 at n = 1, RMSprop update 2.04 at n = 1."""
import math
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch

import heads_ref as H
import parity_util as P

gpu = pytest.mark.gpu
SENT = 7.25          # sentinel of buffers that must stay untouched
OP_TOL = 2e-5        # tests/test_ops_gpu.py close()
INVALID = -1         # DDRL_ERR_INVALID_ARG


# ---- the grid ------------------------------------------------------------------------------------------------------------------
CAT_A = (2, 5, 6, 7, 8, 9, 13, 18)      # the categorical kernels change their weight placement at 6 / 8
GAUSS_D = (1, 2, 3, 8)
BATCHES = (1, 3, 64, 257, 1023, 1024, 1025, 4099)   # 256 workgroups x 4 (8) waves x up to 4 samples: empty workgroups, strides


def _loss_cases():
    """(continuous, A, n, shared, smooth, hyper, B_global): not a full cross, but every A / D with both `shared` and both
    value losses, every batch size with each kernel variant, both B_global, one set of non-default hyper-parameters each."""
    cases = []
    for i, A in enumerate(CAT_A):
        cases.append((0, A, 257, 0, i % 2, "default", 257))
        cases.append((0, A, 64, 1, 1 - i % 2, "default", 3 * 64 + 1))
    for i, n in enumerate(BATCHES):
        for j, A in enumerate((6, 8, 18)):   # LDS rows + transposing reduction, register rows, LDS rows + head_wgrad_kernel
            cases.append((0, A, n, (i + j) % 2, (i + j + 1) % 2 if j else i % 2, "default", n if (i + j) % 2 else 3 * n + 1))
    for D in GAUSS_D:
        for shared in (0, 1):
            for smooth in (0, 1):
                cases.append((1, D, 257, shared, smooth, "default", 257 if smooth else 3 * 257 + 1))
    for i, n in enumerate(BATCHES):
        for j, D in enumerate((2, 8)):
            cases.append((1, D, n, (i + j) % 2, i % 2, "default", 3 * n + 1 if (i + j) % 2 else n))
    cases += [(0, 6, 257, 1, 0, "other", 257), (0, 13, 257, 0, 1, "other", 772), (1, 3, 257, 1, 1, "other", 257),
              (1, 8, 257, 0, 0, "other", 772)]
    out, seen = [], set()
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


LOSS_CASES = _loss_cases()


def _case(spec):
    cont, A, n, shared, smooth, hyper, B = spec
    return H.make_case(cont, A, n, shared, smooth, H.DEFAULT_HYPER if hyper == "default" else H.OTHER_HYPER, seed=1, B_global=B)


def _id(spec):
    cont, A, n, shared, smooth, hyper, B = spec
    return "%s%d-n%d-%s-%s-%s-B%d" % ("gauss" if cont else "cat", A, n, "shared" if shared else "split", "huber" if smooth else "mse", hyper, B)


# ---- CPU: the recipe keeps its promises (runs where there is no GPU) ---------------------------------------------------------------
def test_recipe_reaches_every_branch_with_margin():
    """Every case of the GPU grid: all eight outcomes of the surrogate populated (a fixed subset below 64 samples), every
    float64 ratio more than 1e-3 from 1 - clip, 1 + clip and dual_clip, all three Huber pieces populated and no |err|
    within 1e-3 of 1, faint and exactly-zero advantages present."""
    assert len(LOSS_CASES) >= 70
    for spec in LOSS_CASES:
        H.check_recipe(_case(spec))
    seen = set()
    for spec in LOSS_CASES:
        seen |= {(spec[0], o) for o in _case(spec).outcomes} if spec[2] == 257 else set()
    assert seen == {(f, o) for f in (0, 1) for o in H.OUTCOMES}


def test_reference_gradients_vanish_exactly_where_the_surrogate_is_flat():
    """The float64 reference itself: rows of d(loss)/d(h_actor) are exactly 0 for adv == 0, the dual-clip branch and the
    two clipped-away branches (non-shared, where neither the value nor the entropy gradient reaches h_actor), non-zero elsewhere --
    so that the GPU test's "equal to 0.0" means the branch and not an accident."""
    for spec in ((0, 6, 257, 0, 0, "default", 257), (1, 3, 257, 0, 1, "other", 772)):
        c = _case(spec)
        r = H.loss_block(c, torch.float64)
        flat = torch.tensor([o in ("zero", "neg_dual", "pos_above", "neg_below") for o in c.outcomes])
        rowmax = r["dh_actor"].abs().amax(1)
        assert bool((rowmax[flat] == 0).all()) and bool((rowmax[~flat] > 0).all())
        r32 = H.loss_block(c, torch.float32)
        assert bool(((r32["dh_actor"].abs().amax(1) == 0) == flat).all())


def test_layout_is_as_loose_as_stated():
    for cont, A in ((0, 6), (0, 8), (0, 9), (1, 1), (1, 8)):
        L = H.head_layout(cont, A)
        assert (L["actor_w"] % 4 == 0) == (not cont and A <= 8)
        assert all(L[k] % 4 != 0 for k in ("actor_b", "critic_w", "critic_b")) and (not cont or L["log_std"] % 4 != 0)
        spans = sorted((o, o + cnt) for o, cnt, _ in L["slots"])
        assert all(a[1] < b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] < L["n_params"]   # gaps between all slots


def test_float64_optimiser_restatements_match_torch():
    """heads_ref.adam64 / rmsprop64 are torch.optim.Adam / RMSprop preceded by clip_grad_norm_ (here in float64 on both sides)."""
    n = 300
    p, g, m, v = (t.double() for t in H.optim_inputs(n, 3, "big", 5))
    norm, coef = H.clip_coef64(g, 0.5)
    lr = torch.full((n,), 1e-3, dtype=torch.float64)
    upd, m1, v1, g1 = H.adam64(p, g, m, v, lr, 5, 0.9, 0.999, 1e-8, coef)
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    assert abs(float(torch.nn.utils.clip_grad_norm_([q], 0.5)) - norm) <= 1e-12 * norm
    opt = torch.optim.Adam([q], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    opt.state[q] = {"step": torch.tensor(4.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    assert float((q.detach() - (p + upd)).abs().max()) <= 1e-15 and float((opt.state[q]["exp_avg_sq"] - v1).abs().max()) <= 1e-12 * float(v1.max())
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([q], 0.5)
    opt = torch.optim.RMSprop([q], lr=1e-3, alpha=0.9, eps=1e-8, foreach=False)
    opt.state[q] = {"step": torch.tensor(0.0), "square_avg": v.clone()}
    opt.step()
    upd, sq1, _ = H.rmsprop64(g, v, 1e-3, 0.9, 1e-8, coef)
    assert float((q.detach() - (p + upd)).abs().max()) <= 1e-15 and float((opt.state[q]["square_avg"] - sq1).abs().max()) <= 1e-12 * float(sq1.max())


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def _load():
    from ddrl4nav_amd import _lib
    return _lib, _lib.load()


def _p(t):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def _st():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _desc(c, L):
    from ddrl4nav_amd._lib import HeadsDesc
    d = HeadsDesc()
    d.continuous, d.n_actions, d.shared = int(c.continuous), c.A, int(c.shared)
    for k in ("actor_w", "actor_b", "log_std", "critic_w", "critic_b", "n_params"):
        setattr(d, k, L[k])
    return d


def _cfg(c, **kw):
    from ddrl4nav_amd._lib import default_config
    return default_config(max_batch=c.n, n_actions=max(2, min(c.A, 18)), smooth_l1_loss=int(c.smooth), share_cnn_net=int(c.shared),
                          **c.hyper, **kw)


def close(got, want, tol=OP_TOL):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    scale = max(want.abs().max().item(), 1e-30)
    err = (got - want).abs().max().item()
    assert err <= tol * scale + 1e-7, (err, scale)


MIN_DRAWS = 64


def judge(key, err_k, err_32, draws, where):
    """err_kernel <= 1.25 x err_torch32: the RAW ratio of the two mean errors (both already relative to the quantity's scale)
    is what is asserted and what is recorded -- nothing is subtracted.  Two cases have no ratio and take the operator
    tolerance (OP_TOL, the errors being relative already) instead, openly:
      * a yardstick below the rounding floor (heads_ref.FLOOR): torch's result is correctly rounded, the ratio is noise;
      * fewer than MIN_DRAWS independent draws behind the means (rows with a gradient, samples, elements).  The errors of a row
        share one factor (its log-probability's rounding), so a mean over k rows is a mean of k draws of |noise|: the ratio
        of two such means scatters by about sqrt(2) x 0.75 / sqrt(k), 0.13 at k = 64 and 0.6 at k = 3, against a margin of
        0.25.  The figures of those cases are printed, not judged.  (Non-shared dh_actor has a gradient in about half of the
        rows -- the other outcomes of the surrogate are flat -- so its first judged batch size of the grid is n = 257.)"""
    err_k, err_32 = float(err_k), float(err_32)
    ratio = err_k / err_32 if err_32 > 0 else float("inf")
    print("%-30s kernel %.3e  torch32 %.3e  ratio %-8.3f draws %-7d %s" % (key, err_k, err_32, ratio, draws, where))
    if err_32 > H.FLOOR and draws >= MIN_DRAWS:
        P.MARGINS.check("accuracy", key + "_vs_torch_fp32", ratio, "(%s: kernel %.3e, torch fp32 %.3e)" % (where, err_k, err_32))
    else:
        assert err_k <= OP_TOL, (key, where, err_k, err_32)


def _carve(low, high):
    """Device copies of two host tensors inside ONE allocation, `low` at the lower address (separate allocations land in any order)."""
    buf = torch.cat([low.reshape(-1), high.reshape(-1)]).cuda()
    return buf[:low.numel()].view(low.shape), buf[low.numel():].view(high.shape)


# ---- 1. the loss block ------------------------------------------------------------------------------------------------------------
def run_heads_loss(c, null_dh_critic=False, critic_below=False):
    _lib, lib = _load()
    L = H.head_layout(c.continuous, c.A)
    d = _desc(c, L)
    f = dict(dtype=torch.float32, device="cuda")
    params = H.fill_arena(L, c.params, fill=0.5).cuda()   # finite junk between the slots: nothing may read it into a result
    grads = torch.full((L["n_params"] + 8,), SENT, **f)
    wf = c_int64()
    _lib.check(lib.ddrl_op_heads_ws_floats(byref(d), c.n, byref(wf)))
    ws = torch.zeros(wf.value, **f)
    ha, hc = c.ha.cuda(), c.hc.cuda()
    dh_a = torch.full((c.n + 2, H.FEAT), SENT, **f)
    dh_c = None if null_dh_critic else torch.full((c.n + 2, H.FEAT), SENT, **f)
    if critic_below:     # the critic's features and their gradient at LOWER addresses than the actor's: negative strides in the kernels
        hc, ha = _carve(c.hc, c.ha)
        dh_c, dh_a = _carve(dh_c.cpu(), dh_a.cpu())
        assert hc.data_ptr() < ha.data_ptr() and dh_c.data_ptr() < dh_a.data_ptr()
    cfg = _cfg(c)
    acts, old, adv, ret = (t.contiguous().cuda() for t in (c.actions, c.old_logps, c.advs, c.rets))
    _lib.check(lib.ddrl_op_heads_loss(byref(d), byref(cfg), _p(params), _p(ha), _p(hc), c.n, _p(acts), _p(old), _p(adv), _p(ret),
                                      c.B_global, _p(dh_a), _p(dh_c), _p(grads), _p(ws), _st()))
    torch.cuda.synchronize()
    return {"L": L, "dh_actor": dh_a.cpu(), "dh_critic": None if dh_c is None else dh_c.cpu(), "grads": grads.cpu()}


TINY = 2.0 ** -126   # the smallest normal float32: below it a float32 result has no relative precision left
RATIOS_SEEN = {}     # with row_tol: the largest row error / row tolerance per quantity of this process (a figure to report, no bound)


def check_heads_loss(c, got, where, row_tol=None, fam=None, actor_mass=None):
    """row_tol: per-row relative tolerance (float64 tensor [n]) in place of OP_TOL, for inputs whose rows lose accuracy by a stated
    amount (heads_ref.peaked_row_tol); every whole-tensor quantity -- a sum of row contributions -- then takes the largest of them, and
    a row may miss its float64 value by TINY in absolute terms on top (its float64 gradient may lie below float32's normal range).
    actor_mass (with row_tol; float64 [n]): the magnitude of the terms that cancel inside a row of d(loss)/d(h_actor) -- such a row is
    measured against what entered the difference as well, as the value rows with ret = v are below: row_tol x actor_mass more of
    absolute error, and the row stays out of the mean yardstick where that share is the larger one.
    fam: the family name inside the yardstick keys, so that such inputs keep a record of their own.  The defaults are OP_TOL and the
    head family: what this function has always asserted."""
    r64, r32 = H.loss_block(c, torch.float64), H.loss_block(c, torch.float32)
    fam = fam or ("gauss" if c.continuous else "cat")
    tol_rows = torch.full((c.n,), OP_TOL, dtype=torch.float64) if row_tol is None else row_tol.double()
    tol_all = float(tol_rows.max())
    tiny = 0.0 if row_tol is None else TINY
    L, n, h = got["L"], c.n, c.hyper
    inv_b = 1.0 / c.B_global
    theta = h["v_loss_theta"] if c.shared else 1.0
    # The value gradient of a row is (v - ret) / B x w_c.  One return in seven equals the value to rounding (the recipe's e = 0:
    # |ret - v| < 1e-5 there and > 0.4 everywhere else, heads_ref.check_recipe): in THOSE rows the float64 value gradient is
    # itself rounding noise, so they are measured against what entered the difference (crit_scale) and held to the operator
    # tolerance only.  Every other row is measured against its own largest magnitude and judged beside torch.
    noise = c.err64.abs() < 1e-3
    wc64 = c.params["critic_w"].double()
    hv = (c.ha if c.shared else c.hc).double()
    vmass = (hv.abs() @ wc64.abs()) + c.params["critic_b"].double().abs() + c.rets.double().abs()
    crit_scale = inv_b * theta * vmass * float(wc64.abs().max())
    # rows >= n and everything outside the head slots / the 8-float tail stay as they were
    assert bool((got["dh_actor"][n:] == SENT).all())
    g = got["grads"]
    mask = torch.ones(L["n_params"], dtype=torch.bool)
    for off, cnt, _ in L["slots"]:
        mask[off:off + cnt] = False
    assert bool((g[:L["n_params"]][mask] == SENT).all()), "gradient arena written outside the head slots"
    assert bool(torch.isfinite(g[:L["n_params"]][~mask]).all()) and bool(torch.isfinite(g[L["n_params"]:L["n_params"] + 3]).all())

    # d(loss)/d(features), row by row, each row relative to its own largest magnitude
    def rows(name, key, scale, judged):
        k, w, t = got[name][:n].double(), r64[name], r32[name]
        dead = scale == 0
        if bool(dead.any()):     # no gradient at all in float64: exactly 0.0, not small
            assert bool((k[dead] == 0).all()), (name, where, "rows without gradient must be exactly 0")
        live = ~dead
        if not bool(live.any()):
            return
        ek = (k - w).abs().amax(1) / scale.clamp_min(1e-300)
        et = (t - w).abs().amax(1) / scale.clamp_min(1e-300)
        floor = torch.full((n,), tiny, dtype=torch.float64)
        if actor_mass is not None and name == "dh_actor":
            floor = floor + tol_rows * actor_mass.double()
        allowed = tol_rows + floor / scale.clamp_min(1e-300)
        if row_tol is not None:
            RATIOS_SEEN["heads_%s_%s" % (fam, key)] = max(RATIOS_SEEN.get("heads_%s_%s" % (fam, key), 0.0), float((ek / allowed)[live].max()))
            print("%-30s %s  largest row err / tol %.3f" % ("heads_%s_%s" % (fam, key), where, float((ek / allowed)[live].max())))
        assert bool((ek <= allowed)[live].all()), (name, where, float((ek / allowed)[live].max()), int(((ek / allowed) * live).argmax()))
        sel = live & judged & (tol_rows * scale >= floor)
        if bool(sel.any()):
            judge("heads_%s_%s" % (fam, key), ek[sel].mean(), et[sel].mean(), int(sel.sum()), where)

    rowmax = r64["dh_actor"].abs().amax(1)
    if c.shared:
        rows("dh_actor", "dh_shared", torch.where(noise, torch.maximum(rowmax, crit_scale), rowmax), ~noise)
        if got["dh_critic"] is not None:
            assert bool((got["dh_critic"] == SENT).all()), "shared: dh_critic is not written"
    else:
        rows("dh_actor", "dh_actor", rowmax, torch.ones(n, dtype=torch.bool))
        assert bool((got["dh_critic"][n:] == SENT).all())
        cmax = r64["dh_critic"].abs().amax(1)
        rows("dh_critic", "dh_critic", torch.where(noise, torch.maximum(cmax, crit_scale), cmax), ~noise)

    def slot(name):
        off, cnt = next((o, k) for o, k, nm in L["slots"] if nm == name)
        return g[off:off + cnt].double().reshape(r64["g_" + name].shape)

    # head parameter gradients, per tensor, relative to the tensor's largest magnitude.  The two weight matrices (512 x A and 512
    # numbers, sums over n samples) by their mean error beside torch's ...
    for name in ("actor_w", "critic_w"):
        k, w, t = slot(name), r64["g_" + name], r32["g_" + name]
        scale = float(w.abs().max())
        if scale == 0:
            assert bool((k == 0).all()), (name, where)
            continue
        assert float((k - w).abs().max()) <= tol_all * scale + 1e-7, (name, where)
        judge("heads_%s_g_%s" % (fam, name), (k - w).abs().mean() / scale, (t - w).abs().mean() / scale, n, where)
    # ... the narrow ones (A, 1 or D numbers) and the three loss shares by the operator tolerance: the kernels sum them in
    # double over the workgroups and beat torch's fp32 sum by orders of magnitude, and a handful of numbers is no yardstick
    for name in ("actor_b", "critic_b") + (("log_std",) if c.continuous else ()):
        close(slot(name), r64["g_" + name], tol_all)
    close(g[L["n_params"]:L["n_params"] + 3], r64["losses"], tol_all)
    for i in range(3):   # each share on its own scale as well (the entropy is 20 x the others)
        close(g[L["n_params"] + i:L["n_params"] + i + 1], r64["losses"][i:i + 1], tol_all)


@gpu
@pytest.mark.parametrize("spec", LOSS_CASES, ids=_id)
def test_heads_loss_every_branch_vs_float64(spec):
    """ddrl_op_heads_loss on inputs that take every branch of ppo_surrogate (csrc/ppo_math.h) and every piece of the value
    loss: d(loss)/d(h) per row, the head parameter gradients, the three loss shares, and what must stay untouched."""
    c = _case(spec)
    H.check_recipe(c)
    got = run_heads_loss(c, null_dh_critic=bool(c.shared) and spec[2] % 2 == 1)
    check_heads_loss(c, got, _id(spec))


# ---- 2. acting --------------------------------------------------------------------------------------------------------------------
def run_heads_act(c, act_in, seed=0, stream_id=0, outs=("dist", "action", "logp"), critic_below=False):
    _lib, lib = _load()
    L = H.head_layout(c.continuous, c.A)
    d = _desc(c, L)
    f = dict(dtype=torch.float32, device="cuda")
    params = H.fill_arena(L, c.params, fill=0.5).cuda()
    ha, hc = c.ha.cuda(), c.hc.cuda()
    if critic_below:
        hc, ha = _carve(c.hc, c.ha)
        assert hc.data_ptr() < ha.data_ptr()
    w = c.A
    o = {"dist": torch.full((c.n + 1, w), SENT, **f) if "dist" in outs else None,
         "action": torch.full((c.n + 1, w) if c.continuous else (c.n + 1,), SENT, **f) if "action" in outs else None,
         "logp": torch.full((c.n + 1,), SENT, **f) if "logp" in outs else None, "value": torch.full((c.n + 1,), SENT, **f)}
    a = None if act_in is None else act_in.contiguous().cuda()
    _lib.check(lib.ddrl_op_heads_act(byref(d), _p(params), _p(ha), _p(hc), c.n, _p(a), seed, stream_id, _p(o["dist"]), _p(o["value"]),
                                     _p(o["action"]), _p(o["logp"]), _st()))
    torch.cuda.synchronize()
    out = {k: (None if t is None else t.cpu()) for k, t in o.items()}
    for k, t in out.items():
        if t is not None:
            assert bool((t[c.n:] == SENT).all()), k    # nothing behind the last sample
            out[k] = t[:c.n]
    return out


ACT_CASES = ([(0, A, 257, i % 2) for i, A in enumerate(CAT_A)] + [(0, A, n, (i + 1) % 2) for A in (6, 18) for i, n in enumerate(BATCHES)] +
             [(1, D, 257, s) for D in GAUSS_D for s in (0, 1)] + [(1, 8, n, i % 2) for i, n in enumerate(BATCHES) if n != 257])


@gpu
@pytest.mark.parametrize("spec", ACT_CASES, ids=lambda s: "%s%d-n%d-%s" % ("gauss" if s[0] else "cat", s[1], s[2], "shared" if s[3] else "split"))
def test_heads_act_evaluates_given_actions_vs_float64(spec):
    """ddrl_op_heads_act with act_in: value, probs / mu and the log-probability (categorical: log(clamp(p_hat[a], eps, 1 - eps)),
    Gaussian: the Normal log-density summed over D) against float64, beside torch's fp32 forward.  shared = 1 passes an
    h_critic that points at a DIFFERENT finite buffer: the value is critic(h_actor) all the same (include/ddrl.h)."""
    cont, A, n, shared = spec
    c = H.make_case(cont, A, n, shared, 0, seed=2)
    check_heads_act(c, run_heads_act(c, c.actions), str(spec))


def check_heads_act(c, got, where, row_tol=None, fam=None):
    """row_tol / fam: as check_heads_loss -- the per-row tolerance applies to the rows of `dist`."""
    shared, n = c.shared, c.n
    fam = fam or ("gauss" if c.continuous else "cat")
    ref = {}
    for dt in (torch.float64, torch.float32):
        Pd = {k: v.to(dt) for k, v in c.params.items()}
        ha = c.ha.to(dt)
        dist, logp, _, v, _ = H.forward(c, ha, ha if shared else c.hc.to(dt), Pd, dt)
        ref[dt] = {"dist": dist.double(), "logp": logp.double(), "value": v.double()}
    for k in ("value", "dist", "logp"):
        w, t, kk = ref[torch.float64][k], ref[torch.float32][k], got[k].double().reshape(ref[torch.float64][k].shape)
        scale = float(w.abs().max())
        if k == "dist" and row_tol is not None:
            over = (kk - w).abs().amax(1) / (row_tol.double() * scale + 1e-7)
            RATIOS_SEEN["act_%s_dist" % fam] = max(RATIOS_SEEN.get("act_%s_dist" % fam, 0.0), float(over.max()))
            print("%-30s %s  largest row err / tol %.3f" % ("act_%s_dist" % fam, where, float(over.max())))
            assert float(over.max()) <= 1.0, (k, where, float(over.max()), int(over.argmax()))
        else:
            assert float((kk - w).abs().max()) <= OP_TOL * scale + 1e-7, (k, where)
        judge("act_%s_%s" % (fam, k), (kk - w).abs().mean() / scale, (t - w).abs().mean() / scale, n, where)
    assert bool((got["action"].reshape(c.actions.shape) == c.actions).all())    # the given actions come back


@gpu
@pytest.mark.parametrize("D,n,shared", [(1, 5, 0), (3, 257, 1), (8, 1025, 0)])
def test_gauss_act_sampling_is_consistent_and_reproducible(D, n, shared):
    """act_in == NULL: the returned action is mu + exp(log_std) * z with a finite z, logp_out is the log-density of THAT action,
    the same (seed, stream_id) gives the same bits and another stream_id another draw; NULL outputs are accepted."""
    c = H.make_case(1, D, n, shared, 0, seed=3)
    a = run_heads_act(c, None, seed=11, stream_id=5)
    b = run_heads_act(c, None, seed=11, stream_id=5)
    o = run_heads_act(c, None, seed=11, stream_id=6)
    for k in ("dist", "action", "logp", "value"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["action"], o["action"]) and torch.equal(a["dist"], o["dist"]) and torch.equal(a["value"], o["value"])
    std = torch.exp(c.params["log_std"].double())
    z = (a["action"].double() - a["dist"].double()) / std
    assert bool(torch.isfinite(z).all()) and float(z.abs().max()) < 8.0
    if n * D >= 256:
        assert abs(float(z.mean())) < 0.2 and 0.8 < float(z.std()) < 1.2    # a standard normal, loosely
    want = torch.distributions.Normal(a["dist"].double(), std).log_prob(a["action"].double()).sum(-1)
    close(a["logp"], want)
    only_v = run_heads_act(c, None, seed=11, stream_id=5, outs=())
    assert torch.equal(only_v["value"], a["value"])
    ev = run_heads_act(c, a["action"], outs=("logp",))
    assert torch.equal(ev["logp"], a["logp"]) and torch.equal(ev["value"], a["value"])   # evaluating the drawn action: the same number


@gpu
def test_split_heads_with_the_critic_buffers_below_the_actors():
    """Split encoders, h_critic / dh_critic at LOWER addresses than h_actor / dh_actor (both carved from one tensor, so the order is
    certain): the distance between the two is a stride like any other, negative included.  A = 6, n = 5: two waves' turns, the second
    ragged.  Same float64 restatement and tolerances as the grids above."""
    spec = (0, 6, 5, 0, 0, "default", 5)
    c = _case(spec)
    H.check_recipe(c)
    check_heads_loss(c, run_heads_loss(c, critic_below=True), "critic-below " + _id(spec))
    c = H.make_case(0, 6, 5, 0, 0, seed=2)
    check_heads_act(c, run_heads_act(c, c.actions, critic_below=True), "critic-below act cat6-n5-split")


@gpu
def test_categorical_act_accepts_null_outputs():
    c = H.make_case(0, 6, 37, 1, 0, seed=4)
    full = run_heads_act(c, c.actions)
    part = run_heads_act(c, c.actions, outs=("dist",))
    assert torch.equal(full["value"], part["value"]) and torch.equal(full["dist"], part["dist"])
    s1, s2 = run_heads_act(c, None, seed=3, stream_id=1), run_heads_act(c, None, seed=3, stream_id=1)
    assert torch.equal(s1["action"], s2["action"]) and bool(((s1["action"] >= 0) & (s1["action"] < 6)).all())


# ---- 3. optimiser steps -------------------------------------------------------------------------------------------------------------
BIG = 2048 * 256 + 3      # more than one pass of the 2,048-workgroup grid
F32 = lambda x: float(np.float32(x))     # the hyper-parameters ARE the floats ddrl_config carries


def _adam_cases():
    cases = []
    steps, kinds = (1, 2, 1000, 200000), ("big", "small", "big", "big")
    i = 0
    for n in (1, 255, 257, BIG):
        for na in sorted({0, 1, (n // 2) | 1 if n > 2 else 1, n}):
            cases.append((n, min(na, n), 0, steps[i % 4], kinds[(i // 2) % 4], 1))
            i += 1
    cases += [(257, 100, 1, 2, "big", 1), (BIG, 7, 1, 1000, "small", 1), (255, 101, 0, 1, "zero", 1), (BIG, 1001, 0, 1, "zero", 1),
              (257, 129, 0, 2, "big", 0), (255, 0, 0, 200000, "small", 0), (257, 255, 0, 1000, "small", 1)]
    return cases


def _torch_adam32(p, g, m, v, parts, step, betas, eps, clip, max_norm):
    ps = [torch.nn.Parameter(p[a:b].clone()) for a, b, _ in parts]
    for q, (a, b, _) in zip(ps, parts):
        q.grad = g[a:b].clone()
    if clip:
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
    opt = torch.optim.Adam([{"params": [q], "lr": lr} for q, (_, _, lr) in zip(ps, parts)], betas=betas, eps=eps, foreach=False)
    for q, (a, b, _) in zip(ps, parts):
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m[a:b].clone(), "exp_avg_sq": v[a:b].clone()}
    opt.step()
    cat = lambda f: torch.cat([f(q) for q in ps]).detach().double()
    return cat(lambda q: q.data), cat(lambda q: opt.state[q]["exp_avg"]), cat(lambda q: opt.state[q]["exp_avg_sq"])


def _elementwise(key, k, w, t, scale, n, where):
    """mean of the element-wise errors relative to `scale` (float64, per element); scale 0 = the element must be exact."""
    dead = scale == 0
    if bool(dead.any()):
        assert bool((k[dead] == w[dead]).all()), (key, where)
    live = ~dead
    if bool(live.any()):
        ek, et = ((k - w).abs() / scale.clamp_min(1e-300))[live], ((t - w).abs() / scale.clamp_min(1e-300))[live]
        assert float(ek.max()) <= OP_TOL, (key, where, float(ek.max()))
        judge(key, ek.mean(), et.mean(), int(live.sum()), where)


@gpu
@pytest.mark.parametrize("case", _adam_cases(), ids=lambda c: "n%d-na%d-%s-step%d-%s-%s" % (c[0], c[1], "shared" if c[2] else "two_lr", c[3], c[4], "clip" if c[5] else "noclip"))
def test_clip_adam_one_step_element_by_element(case):
    """ddrl_op_clip_adam, ONE step: the norm, the coefficient, the total loss, the gradient scaled in place, both moments and
    the parameter update of every element against float64, beside torch.optim.Adam(foreach=False) on the CPU in fp32."""
    _lib, lib = _load()
    n, n_actor, shared, step, kind, clip = case
    where = str(case)
    p, g, m, v = H.optim_inputs(n, 7 * n + n_actor + step, kind, step)
    for i in (n_actor - 1, n_actor):     # the two sides of the learning-rate boundary: zero parameter, solid gradient
        if 0 <= i < n:
            p[i] = 0.0
            if kind != "zero":
                g[i] = g.abs().max() * (0.5 if i % 2 else -0.5)
    cfg = _lib.default_config(clip_grad=clip)
    b1, b2, eps, max_norm = F32(cfg.adam_beta1), F32(cfg.adam_beta2), F32(cfg.adam_eps), F32(cfg.clip_grad_norm)
    assert cfg.critic_lr == pytest.approx(20 * cfg.actor_lr)
    if shared:
        parts = [(0, n, F32(cfg.learning_rate))]
    else:
        parts = [x for x in ((0, n_actor, F32(cfg.actor_lr)), (n_actor, n, F32(cfg.critic_lr))) if x[1] > x[0]]
    lr = torch.cat([torch.full((b - a,), l, dtype=torch.float64) for a, b, l in parts])
    tail = torch.tensor([0.37, 1.91, 0.83, SENT, SENT, SENT, SENT, SENT])
    f = dict(dtype=torch.float32, device="cuda")
    gd = torch.cat([g, tail]).cuda()
    pd, md, vd = p.cuda(), m.cuda(), v.cuda()
    wb = c_int64()
    _lib.check(lib.ddrl_op_clip_adam_ws_bytes(byref(wb)))
    ws = torch.zeros(wb.value, dtype=torch.uint8, device="cuda")
    _lib.check(lib.ddrl_op_clip_adam(byref(cfg), _p(pd), _p(gd), _p(md), _p(vd), n, n_actor, shared, step, _p(ws), _st()))
    torch.cuda.synchronize()
    gk, pk, mk, vk = gd.cpu(), pd.cpu().double(), md.cpu().double(), vd.cpu().double()
    norm64, coef64 = H.clip_coef64(g.double(), max_norm, bool(clip))
    assert abs(float(gk[n + 4]) - norm64) <= 2.0 ** -24 * norm64 * (1 + 1e-6), (float(gk[n + 4]), norm64)   # one fp32 rounding
    coef_k = float(gk[n + 5])
    if kind in ("small", "zero") or not clip:
        assert coef_k == 1.0 and torch.equal(gk[:n], g)       # nothing to clip: the gradient keeps its bits
    else:
        assert coef64 < 0.1 and abs(coef_k - coef64) <= 2.0 ** -22 * coef64    # three fp32 roundings: norm, norm + 1e-6, the quotient
        assert torch.equal(gk[:n], g * np.float32(coef_k))     # scaled in place by the coefficient it reports
    want_total = 0.37 + 1.91 * F32(cfg.v_loss_theta) - 0.83 * F32(cfg.ent_loss_theta)
    assert abs(float(gk[n + 3]) - want_total) <= 2.0 ** -23 * (0.37 + 1.91 + 0.83)
    assert torch.equal(gk[n:n + 3], tail[:3]) and bool((gk[n + 6:] == SENT).all())
    upd64, m64, v64, g64 = H.adam64(p.double(), g.double(), m.double(), v.double(), lr, step, b1, b2, eps, coef64)
    p32, m32, v32 = _torch_adam32(p, g, m, v, parts, step, (b1, b2), eps, clip, max_norm)
    assert bool(torch.isfinite(pk).all() and torch.isfinite(mk).all() and torch.isfinite(vk).all())
    if kind == "zero":
        assert torch.equal(pk, p.double()) and bool((mk == 0).all()) and bool((vk == 0).all())    # nothing moves, nothing is NaN
        return
    _elementwise("adam_m", mk, m64, m32, torch.maximum(m.double().abs(), g64.abs()), n, where)
    _elementwise("adam_v", vk, v64, v32, v64, n, where)
    step_lr = lr / (1.0 - b1 ** step)
    zero_p = p == 0
    for sel, key in ((zero_p, "adam_update"), (~zero_p, "adam_update_rounded_into_p")):
        if bool(sel.any()):
            # relative to lr -- or to the update itself where it is larger (a second moment of exactly 0 under a running first moment
            # gives updates of thousands of lr: fp32 resolves those to THEIR last place) -- and, where the update is rounded into a
            # non-zero parameter, to the larger of the two numbers added
            _elementwise(key, (pk - p.double())[sel], upd64[sel], (p32 - p.double())[sel],
                         torch.maximum(torch.maximum(step_lr, upd64.abs()), p.double().abs())[sel], n, where)
    for i in (n_actor - 1, n_actor):     # each side of the boundary moved with ITS learning rate (they differ 20-fold)
        if 0 <= i < n and not shared:
            assert abs(float(pk[i]) - float(upd64[i])) <= 1e-3 * abs(float(upd64[i])), (i, float(pk[i]), float(upd64[i]))


@gpu
@pytest.mark.parametrize("n,kind,fresh", [(1, "big", 1), (255, "big", 0), (257, "small", 0), (BIG, "big", 0), (BIG, "small", 1), (257, "zero", 1)])
def test_clip_rmsprop_one_step_element_by_element(n, kind, fresh):
    _lib, lib = _load()
    where = "n%d-%s-%s" % (n, kind, "fresh" if fresh else "running")
    p, g, _, sq = H.optim_inputs(n, 11 * n + fresh, kind, 1 if fresh else 9)
    lr, alpha, eps, max_norm = F32(5e-5), 0.9, F32(1e-8), F32(0.01 if kind == "big" else 1.0)
    gd = torch.cat([g, torch.full((8,), SENT)]).cuda()
    pd, sd = p.cuda(), sq.cuda()
    wb = c_int64()
    _lib.check(lib.ddrl_op_clip_adam_ws_bytes(byref(wb)))      # "ws: as ddrl_op_clip_adam" (include/ddrl.h)
    ws = torch.zeros(wb.value, dtype=torch.uint8, device="cuda")
    _lib.check(lib.ddrl_op_clip_rmsprop(_p(pd), _p(gd), _p(sd), n, lr, alpha, eps, max_norm, _p(ws), _st()))
    torch.cuda.synchronize()
    gk, pk, sk = gd.cpu(), pd.cpu().double(), sd.cpu().double()
    norm64, coef64 = H.clip_coef64(g.double(), max_norm)
    assert abs(float(gk[n + 4]) - norm64) <= 2.0 ** -24 * norm64 * (1 + 1e-6)
    coef_k = float(gk[n + 5])
    if kind == "big":
        assert coef64 < 0.5 and abs(coef_k - coef64) <= 2.0 ** -22 * coef64 and torch.equal(gk[:n], g * np.float32(coef_k))
    else:
        assert coef_k == 1.0 and torch.equal(gk[:n], g)
    assert bool((gk[n:n + 4] == SENT).all()) and bool((gk[n + 6:] == SENT).all())
    upd64, sq64, g64 = H.rmsprop64(g.double(), sq.double(), lr, alpha, eps, coef64)
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([q], max_norm)
    opt = torch.optim.RMSprop([q], lr=lr, alpha=alpha, eps=eps, foreach=False)
    opt.state[q] = {"step": torch.tensor(0.0), "square_avg": sq.clone()}
    opt.step()
    if kind == "zero":
        assert torch.equal(pk, p.double()) and bool((sk == 0).all())
        return
    _elementwise("rmsprop_square_avg", sk, sq64, opt.state[q]["square_avg"].double(), sq64, n, where)
    zero_p = p == 0
    _elementwise("rmsprop_update", (pk - p.double())[zero_p], upd64[zero_p], (q.detach().double() - p.double())[zero_p],
                 upd64[zero_p].abs().clamp_min(lr), n, where) if bool(zero_p.any()) else None
    if kind == "small":
        # coefficient exactly 1 on both sides; alpha and 1 - alpha each cast to fp32 once, as torch casts them (1.0f - 0.9f is 2 - 4 ulp
        # off).  Fresh square_avg: (float(1 - alpha) g) g on both sides, the same bits.  Running: torch's CPU addcmul may fuse into one
        # fma where the library rounds the product first -- one ulp apart on about a tenth of the elements.
        bits_k, bits_t = sd.cpu().view(torch.int32), opt.state[q]["square_avg"].view(torch.int32)
        if fresh:
            assert torch.equal(bits_k, bits_t)
        else:
            assert int((bits_k - bits_t).abs().max()) <= 1


# ---- 4. the remaining small operators --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,ld,shared,smooth,null", [(1, 512, 0, 0, ""), (5, 520, 1, 1, "dw"), (1025, 520, 0, 1, "db"), (4099, 512, 1, 0, "vloss"),
                                                     (4099, 520, 0, 0, ""), (1025, 512, 1, 1, "dw,db")])
def test_value_head_forward_and_loss(n, ld, shared, smooth, null):
    _lib, lib = _load()
    g = torch.Generator().manual_seed(n + ld)
    B = 2 * n + 3
    arena = torch.full((530,), 0.5)
    w, b = torch.randn(512, generator=g) * 0.05, torch.randn(1, generator=g) * 0.1
    arena[5:517], arena[519:520] = w, b          # 4-byte aligned, not 16-byte aligned
    h = torch.full((n, ld), 3e30)                # padding columns hold large finite junk
    h[:, :512] = torch.randn(n, 512, generator=g) * 0.5
    v64 = h[:, :512].double() @ w.double() + b.double()
    e = torch.tensor([H.HUBER_E[i % 7] for i in range(n)], dtype=torch.float64) * 1.03
    rets = (v64 + e).float()
    ad, hd, rd = arena.cuda(), h.cuda(), rets.cuda()
    value = torch.full((n + 1,), SENT, device="cuda")
    _lib.check(lib.ddrl_op_value_head_forward(_p(ad[5:]), _p(ad[519:]), _p(hd), ld, n, _p(value), _st()))
    close(value[:n], v64)
    assert float(value[n]) == SENT
    cfg = _lib.default_config(smooth_l1_loss=smooth, v_loss_theta=0.5)
    err = rets.double() - v64
    if smooth:
        el, gv = torch.where(err.abs() < 1, 0.5 * err * err, err.abs() - 0.5), -err.clamp(-1, 1)
    else:
        el, gv = 0.5 * err * err, -err
    gv = gv / B * (0.5 if shared else 1.0)
    dh0 = torch.full((n + 1, ld), SENT)
    dh0[:n, :512] = torch.randn(n, 512, generator=g) * (0.05 / B)     # the gradient is ADDED to what is there, at its own magnitude
    dhd = dh0.cuda()
    wf = c_int64()
    _lib.check(lib.ddrl_op_value_head_ws_floats(byref(wf)))
    ws = torch.zeros(wf.value, device="cuda")
    out = torch.full((520,), SENT, device="cuda")      # dw at 1 (4-byte aligned), db at 515, the loss accumulator at 517 pre-filled
    out[517] = 0.25
    dw = None if "dw" in null else out[1:]
    db = None if "db" in null else out[515:]
    acc = None if "vloss" in null else out[517:]
    _lib.check(lib.ddrl_op_value_head_loss(byref(cfg), shared, _p(ad[5:]), _p(ad[519:]), _p(hd), ld, n, _p(rd), B, _p(dhd), ld, _p(dw), _p(db),
                                           _p(acc), _p(ws), _st()))
    torch.cuda.synchronize()
    got, o = dhd.cpu(), out.cpu()
    close(got[:n, :512], dh0[:n, :512].double() + gv[:, None] * w.double()[None, :])
    assert bool((got[:, 512:] == SENT).all()) and bool((got[n] == SENT).all())       # columns 512.. and the row behind the batch
    if dw is not None:
        close(o[1:513], gv @ h[:, :512].double())
    else:
        assert bool((o[1:513] == SENT).all())
    if db is not None:
        close(o[515:516], gv.sum().reshape(1))
    else:
        assert float(o[515]) == SENT
    if acc is not None:
        close(o[517:518], (0.25 + el.sum() / B).reshape(1))
    else:
        assert float(o[517]) == 0.25
    assert float(o[0]) == SENT and float(o[513]) == SENT and float(o[516]) == SENT and bool((o[518:] == SENT).all())


@gpu
@pytest.mark.parametrize("n,n_total,width,ld,ld_d,sign,acc", [(1, 1, 1, 1, 1, 1.0, 0), (300, 300, 4, 4, 4, -1.0, 0), (257, 1000, 7, 9, 12, 1.0, 1),
                                                             (1000, 1001, 1, 3, 2, -1.0, 1), (77, 77, 7, 7, 8, -1.0, 0)])
def test_wgan_terms(n, n_total, width, ld, ld_d, sign, acc):
    _lib, lib = _load()
    g = torch.Generator().manual_seed(n + width)
    score = torch.randn(n + 1, ld, generator=g)
    ds = torch.full((n + 1, ld_d), SENT, device="cuda")
    loss = torch.tensor([0.75, SENT], device="cuda")
    sd = score.cuda()
    _lib.check(lib.ddrl_op_wgan_terms(_p(sd), ld, n, n_total, sign, _p(ds), ld_d, width, _p(loss), acc, _st()))
    torch.cuda.synchronize()
    d = ds.cpu()
    assert torch.equal(d[:n, 0], torch.full((n,), float(np.float32(sign) / np.float32(n_total))))     # bit-exactly sign / n_total
    assert bool((d[:n, 1:width] == 0).all()) and bool((d[:n, width:] == SENT).all()) and bool((d[n] == SENT).all())
    want = sign * math.fsum(score[:n, 0].double().tolist()) / n_total + (0.75 if acc else 0.0)
    assert abs(float(loss[0]) - want) <= 2.0 ** -23 * (abs(want) + (0.75 if acc else 0.0)) + 1e-12 and float(loss[1]) == SENT


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536])
@pytest.mark.parametrize("width,ld", [(1, 1), (3, 5), (1, 4)])
def test_colsum_is_correctly_rounded_and_cancels(n, width, ld):
    _lib, lib = _load()
    g = torch.Generator().manual_seed(n + ld)
    x = torch.randn(n, ld, generator=g) * 10.0 ** (torch.rand(n, ld, generator=g) * 6 - 3)
    out = torch.full((width + 1,), SENT, device="cuda")
    xd = x.cuda()
    _lib.check(lib.ddrl_op_colsum(_p(xd), ld, n, width, _p(out), _st()))
    o = out.cpu()
    for cidx in range(width):
        want = math.fsum(x[:, cidx].double().tolist())
        assert abs(float(o[cidx]) - want) <= 2.0 ** -24 * abs(want) * (1 + 1e-6) + 1e-45, (cidx, float(o[cidx]), want)   # one fp32 rounding
    assert float(o[width]) == SENT
    c0 = float(np.float32(1.0) / np.float32(n + 2))       # the WGAN bias gradient: +c over the rows and -c over the same rows
    plus, minus = torch.full((n, ld), c0).cuda(), torch.full((n, ld), -c0).cuda()
    op, om = torch.empty(width, device="cuda"), torch.empty(width, device="cuda")
    _lib.check(lib.ddrl_op_colsum(_p(plus), ld, n, width, _p(op), _st()))
    _lib.check(lib.ddrl_op_colsum(_p(minus), ld, n, width, _p(om), _st()))
    assert bool(((op + om) == 0).all()) and abs(float(op[0]) - n * c0) <= 2.0 ** -24 * n * c0 * (1 + 1e-6)


@gpu
@pytest.mark.parametrize("n,width,ld_d,ld_act", [(1, 1, 1, 1), (37, 7, 7, 7), (300, 7, 9, 12), (5, 513, 516, 513)])
def test_relu_mask_keeps_bits_and_writes_plus_zero(n, width, ld_d, ld_act):
    _lib, lib = _load()
    g = torch.Generator().manual_seed(n + width)
    vals = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1.5, -2.0, 3e-38])
    act = vals[torch.randint(0, 7, (n, ld_act), generator=g)]
    d = torch.randn(n, ld_d, generator=g) * 10.0 ** (torch.rand(n, ld_d, generator=g) * 20 - 10)
    d[:, 0] = -0.0 if n > 1 else d[:, 0]
    dd, ad = d.clone().cuda(), act.cuda()
    _lib.check(lib.ddrl_op_relu_mask(_p(dd), ld_d, _p(ad), ld_act, n, width, _st()))
    got = dd.cpu()
    keep = act[:, :width] > 0
    assert torch.equal(got[:, :width][keep].view(torch.int32), d[:, :width][keep].view(torch.int32))      # kept bit-exactly
    masked = got[:, :width][~keep]
    assert bool((masked == 0).all()) and not bool(torch.signbit(masked).any())                              # +0.0, not -0.0
    assert torch.equal(got[:, width:].view(torch.int32), d[:, width:].view(torch.int32))                  # padding untouched


@gpu
@pytest.mark.parametrize("count", [1, 255, 4096 * 256 + 5])
@pytest.mark.parametrize("dst_off,src_off", [(0, 0), (1, 0), (1, 3)])
def test_accumulate_is_the_fp32_sum_at_any_float_offset(count, dst_off, src_off):
    """include/ddrl.h states no alignment rule for ddrl_op_accumulate, and the kernel needs none (4-byte loads and stores)."""
    _lib, lib = _load()
    g = torch.Generator().manual_seed(count)
    dst = torch.randn(count + 8, generator=g)
    src = torch.randn(count + 8, generator=g) * 10.0 ** (torch.rand(count + 8, generator=g) * 8 - 4)
    dd, sd = dst.clone().cuda(), src.cuda()
    _lib.check(lib.ddrl_op_accumulate(_p(dd[dst_off:]), _p(sd[src_off:]), count, _st()))
    want = dst.clone()
    want[dst_off:dst_off + count] += src[src_off:src_off + count]
    assert torch.equal(dd.cpu().view(torch.int32), want.view(torch.int32))


@gpu
@pytest.mark.parametrize("n", [1, 5, 300])
@pytest.mark.parametrize("width,ld", [(1, 4), (5, 8), (773, 776), (773, 800)])
def test_row_amax_is_exact_and_ignores_padding(n, width, ld):
    _lib, lib = _load()
    g = torch.Generator().manual_seed(n + width + ld)
    x = torch.full((n, ld), -3e30)                    # large finite values in the padding columns [width, ld)
    x[:, :width] = torch.randn(n, width, generator=g) * 10.0 ** (torch.rand(n, 1, generator=g) * 8 - 4)
    if n > 2:
        x[1, :width] = 0.0
    want = x[:, :width].abs().amax(1)
    xd = x.cuda()
    out = torch.full((n + 1,), SENT, device="cuda")
    _lib.check(lib.ddrl_op_row_amax(_p(xd), ld, width, n, _p(out), 0, _st()))
    assert torch.equal(out.cpu()[:n], want) and float(out[n]) == SENT
    pre = want.clone()
    pre[::2] = pre[::2] * 4.0 + 1.0                   # slots already raised above the row: never lowered; the others: raised to it
    pre[1::2] = pre[1::2] * 0.25
    acc = pre.clone().cuda()
    _lib.check(lib.ddrl_op_row_amax(_p(xd), ld, width, n, _p(acc), 1, _st()))
    assert torch.equal(acc.cpu(), torch.maximum(pre, want))


@gpu
@pytest.mark.parametrize("n,elems,sn", [(1, 4, 4), (5, 8, 12), (300, 772, 772), (37, 772, 800), (3, 4100, 4104)])
def test_sample_amax_is_exact_and_ignores_what_lies_between_samples(n, elems, sn):
    _lib, lib = _load()
    g = torch.Generator().manual_seed(n + elems)
    x = torch.full((n, sn), 3e30)                     # garbage between the samples
    x[:, :elems] = torch.randn(n, elems, generator=g) * 10.0 ** (torch.rand(n, 1, generator=g) * 8 - 4)
    xd = x.cuda()
    out = torch.full((n + 1,), SENT, device="cuda")
    _lib.check(lib.ddrl_op_sample_amax(_p(xd), sn, elems, n, _p(out), _st()))
    assert torch.equal(out.cpu()[:n], x[:, :elems].abs().amax(1)) and float(out[n]) == SENT


@gpu
def test_argument_checks_answer_before_any_launch():
    """Every call below is refused with DDRL_ERR_INVALID_ARG by the argument checks, which run before anything touches HIP."""
    _lib, lib = _load()
    c = H.make_case(0, 6, 8, 0, 0, seed=5)
    L = H.head_layout(0, 6)
    cfg = _cfg(c)
    buf = torch.zeros(16384, device="cuda")
    a = _p(buf)
    off4 = c_void_p(buf.data_ptr() + 4)               # 4-byte aligned, not 16-byte aligned
    st = _st()

    def loss(d, n=8, B=8, ha=a):
        return lib.ddrl_op_heads_loss(byref(d), byref(cfg), a, ha, a, n, a, a, a, a, B, a, a, a, a, st)

    def act(d, n=8, ha=a):
        return lib.ddrl_op_heads_act(byref(d), a, ha, a, n, a, 0, 0, a, a, a, a, st)

    def desc(cont, A):
        cc = H.Case()
        cc.continuous, cc.A, cc.shared = cont, A, 0
        return _desc(cc, L)
    ok = desc(0, 6)
    assert loss(ok, n=0) == INVALID and act(ok, n=0) == INVALID
    assert loss(ok, n=8, B=7) == INVALID
    for cont, A in ((0, 1), (0, 19), (1, 0), (1, 9)):
        assert loss(desc(cont, A)) == INVALID and act(desc(cont, A)) == INVALID, (cont, A)
        wf = c_int64()
        assert lib.ddrl_op_heads_ws_floats(byref(desc(cont, A)), 8, byref(wf)) == INVALID
    assert loss(ok, ha=off4) == INVALID and act(ok, ha=off4) == INVALID
    assert lib.ddrl_op_value_head_forward(a, a, a, 510, 8, a, st) == INVALID
    assert lib.ddrl_op_value_head_loss(byref(cfg), 0, a, a, a, 510, 8, a, 8, a, 512, a, a, a, a, st) == INVALID
    assert lib.ddrl_op_value_head_loss(byref(cfg), 0, a, a, a, 512, 8, a, 7, a, 512, a, a, a, a, st) == INVALID
    assert lib.ddrl_op_clip_adam(byref(cfg), a, a, a, a, 100, 10, 0, 0, a, st) == INVALID       # step = 0
    assert lib.ddrl_op_clip_adam(byref(cfg), a, a, a, a, 100, 101, 0, 1, a, st) == INVALID     # n_actor > n_params
    assert lib.ddrl_op_sample_amax(a, 8, 6, 2, a, st) == INVALID                                # elems not a multiple of 4
    assert lib.ddrl_op_sample_amax(off4, 8, 8, 2, a, st) == INVALID
    assert lib.ddrl_op_row_amax(a, 6, 5, 2, a, 0, st) == INVALID                                # ld not a multiple of 4
    assert lib.ddrl_op_wgan_terms(a, 1, 8, 7, 1.0, a, 1, 1, a, 0, st) == INVALID                # n_total < n
    assert lib.ddrl_op_colsum(a, 2, 8, 3, a, st) == INVALID and lib.ddrl_op_relu_mask(a, 3, a, 4, 8, 4, st) == INVALID
    assert lib.ddrl_op_accumulate(a, a, 0, st) == INVALID
    torch.cuda.synchronize()
