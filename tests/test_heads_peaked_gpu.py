"""The categorical head kernels on peaked, saturated and collapsed policies (csrc/heads.hip, csrc/heads_common.h, csrc/diag.hip): the
closed-interval clamps of log(clamp(q, eps, 1 - eps)) and the two gradient gates behind them, expf in its subnormal range and at
underflow, rows whose whole actor gradient is exactly zero because the policy is saturated, ratios of 2^+-20, sampling from rows with
q_j == 0 -- none of which the near-uniform recipe of tests/test_heads_optim_ops_gpu.py reaches.  Inputs: heads_ref.make_peaked_case (its
promises: tests/test_heads_peaked_cpu.py); reference: float64, through check_heads_loss / check_heads_act of
tests/test_heads_optim_ops_gpu.py with the per-row tolerance heads_ref.peaked_row_tol, OP_TOL + 8 ulp32(max_j |z_bj|), and yardstick keys of
their own (heads_cat_peaked_*, act_cat_peaked_*).  Then a policy is driven into collapse -- by the operators on fixed features, and by
the whole Atari context on fixed frames -- and every statistic and gradient on the way has to stay finite.

A row on the boundary itself (q_top == 1 - eps to the bit in float32, inside the interval in float64) is the one place where an open
interval in a gate differs from the closed one; heads_peaked_ref.make_boundary_case goes there from the side on which float32 and
float64 agree.  The lower boundary (q_j == eps to the bit) cannot be placed through logits -- one ulp of a logit near 16 moves q_j by
sixteen of its own ulps -- and q = p / sum(p) differs from p by rounding only (sum(p) = 1 +- A 2^-24).

Measured on an MI355X, largest row error / row tolerance over the grids: heads_cat_peaked_dh_actor 0.112, dh_shared 0.109, dh_critic
0.014, act_cat_peaked_dist 0.018; the boundary rows are off by less than 5e-5 of the row (bounds 0.2 and 0.03); the underflow cases come
back with subnormal probabilities and with zeros (cat18-n257: 2,193 and 2,176).  Both collapse loops end at an entropy of 1.192e-07 =
-log(1 - eps), the operator loop after passing 1.5e-7 at step 6 exactly as float64 does.  The context loop returned NaN at its 22nd
iteration until the plane scales were bounded (common.h PLANE_SCALE_EXP_MAX).

Mutations of csrc/heads.hip / heads_common.h, each run once against this file and the earlier tests of the head kernels
(tests/test_heads_optim_ops_gpu.py, the heads_loss_opt and context tests of tests/test_loss_options_gpu.py, the operator tests of
tests/test_ppo_diag_gpu.py); no earlier test failed under any of them:
  g_qa `qa <= 1 - eps` -> `<`      4 failed: test_the_gates_are_closed_intervals_at_the_upper_boundary, every A
  inr  `qj <= 1 - eps` -> `<`      4 failed: the same four
  logp_out without the clamp       20 failed: test_heads_act_evaluates_actions_of_peaked_policies, every case
  g_qa `qa >= eps` -> `>`          nothing failed   } q_j == eps to the bit does not occur in any case (see above): these two
  inr  `qj >= eps` -> `>`          nothing failed   } comparisons are not pinned down by the suite
  d.q[j] = d.p[j] (no / d.ps)      nothing failed: a change of the last bit, below every tolerance here
"""
import math
from ctypes import byref, c_int64

import numpy as np
import pytest
import torch

import heads_peaked_ref as R
import heads_ref as H
import loss_options_ref as LR
import test_heads_optim_ops_gpu as T

pytestmark = pytest.mark.gpu

FAM = "cat_peaked"
GRID, OPT_GRID = R.grid(), R.opt_grid()
LOG_EPS32 = float(np.float32(math.log(2.0 ** -23)))               # what a clamped-from-below probability's logarithm is
LOG_TOP32 = float(np.float32(math.log(1.0 - 2.0 ** -23)))         # ... and a clamped-from-above one's


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for k, v in sorted(T.RATIOS_SEEN.items()):
        print("largest row error / row tolerance  %-32s %.3f" % (k, v))


def _check_loss(c, got, where):
    T.check_heads_loss(c, got, where, row_tol=R.row_tol(c), fam=FAM, actor_mass=R.entropy_mass(c))
    for k in ("dh_actor", "dh_critic", "grads"):
        if got[k] is not None:
            t = got[k]
            assert bool(torch.isfinite(t[t != T.SENT]).all()), (k, where)


# ---- 1. the loss block ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", GRID, ids=R.case_id)
def test_heads_loss_on_peaked_policies_vs_float64(spec):
    """ddrl_op_heads_loss: d(loss)/d(h) per row, the head gradients, the three loss shares, exact zeros where float64 has no gradient
    (saturated rows of split encoders among them), untouched sentinels."""
    c = R.case_of(spec)
    H.check_peaked_recipe(c)
    _check_loss(c, T.run_heads_loss(c, null_dh_critic=bool(c.shared) and spec[1] % 2 == 1), R.case_id(spec))


@pytest.mark.parametrize("spec", OPT_GRID, ids=R.case_id)
def test_heads_loss_opt_on_peaked_policies_vs_float64(spec, monkeypatch):
    """ddrl_op_heads_loss_opt with the option sets `entropy` and `both`, split encoders above all: the entropy gradient through both
    clamps (log(clamp(q_j)) and q_j / clamp(q_j)) on rows whose q_j are below eps, subnormal or 0."""
    from test_loss_options_gpu import run_heads_loss_opt
    c = R.case_of(spec)
    H.check_peaked_recipe(c)
    monkeypatch.setattr(T.H, "loss_block", LR.loss_block)
    _check_loss(c, run_heads_loss_opt(c), R.case_id(spec))


# ---- 2. on the closed upper boundary ----------------------------------------------------------------------------------------------------
def _boundary_rows(c, got, r64, where):
    """Per row: largest error of d(loss)/d(h_actor) relative to the row's largest float64 magnitude (inf where float64 has none)."""
    k, w = got["dh_actor"][:c.n].double(), r64["dh_actor"]
    assert bool(torch.isfinite(k).all()), where
    return (k - w).abs().amax(1) / w.abs().amax(1)


@pytest.mark.parametrize("A", R.SIZES)
def test_the_gates_are_closed_intervals_at_the_upper_boundary(A):
    """q_top == 1 - eps exactly: the surrogate's gradient of a row that took `top` passes (split encoders: it is the whole row), and
    under the split entropy bonus the rows with a zero advantage carry the entropy gradient with q_top / clamp(q_top) = 1.  Bounds:
    heads_peaked_ref.BOUNDARY_ACTOR_TOL / BOUNDARY_ENTROPY_TOL -- what float32 cannot know about 1 - q_top, worked out there."""
    from test_loss_options_gpu import run_heads_loss_opt
    c = R.make_boundary_case(A, 9, 0)
    R.check_boundary_case(c)
    err = _boundary_rows(c, T.run_heads_loss(c), H.loss_block(c, torch.float64), "plain")
    print("A = %d: rows that took top, actor gradient: largest error %.4f of the row" % (A, float(err[c.took].max())))
    assert bool((err[c.took] <= R.BOUNDARY_ACTOR_TOL).all()), (A, err[c.took].tolist())
    assert bool((T.run_heads_loss(c)["dh_actor"][:c.n][~c.took] == 0).all())          # advantage 0, no entropy term: nothing
    LR.attach_options(c, LR.OPTION_SETS["entropy"])
    err = _boundary_rows(c, run_heads_loss_opt(c), LR.loss_block(c, torch.float64), "entropy")
    print("A = %d: rows with a zero advantage, entropy gradient: largest error %.4f of the row" % (A, float(err[~c.took].max())))
    assert bool((err[~c.took] <= R.BOUNDARY_ENTROPY_TOL).all()), (A, err[~c.took].tolist())


# ---- 3. acting ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", GRID, ids=R.case_id)
def test_heads_act_evaluates_actions_of_peaked_policies(spec):
    """ddrl_op_heads_act with act_in: probs, value and log-probability against float64; an action with q < eps comes back with exactly
    float32(log(2^-23)) and one with q > 1 - eps with exactly float32(log(1 - 2^-23)): both are the clamp's value, not a rounding."""
    c = R.case_of(spec)
    got = T.run_heads_act(c, c.actions)
    T.check_heads_act(c, got, R.case_id(spec), row_tol=R.row_tol(c), fam=FAM)
    q = torch.softmax(c.z64, -1).gather(1, c.actions.long()[:, None])[:, 0]
    low, high = q < H.CAT_EPS, q > 1.0 - H.CAT_EPS
    assert bool((got["logp"][low] == LOG_EPS32).all()), got["logp"][low].tolist()[:4]
    assert bool((got["logp"][high] == LOG_TOP32).all()), got["logp"][high].tolist()[:4]
    assert bool(torch.isfinite(got["dist"]).all()) and bool((got["dist"] >= 0).all())
    if c.n >= 64:
        assert bool(low.any()) and bool(high.any())
        if spec[4] == "underflow":
            tail = got["dist"][got["dist"] < 0.5]
            print("%s: %d subnormal and %d zero probabilities returned" % (R.case_id(spec), int(((tail > 0) & (tail < 2.0 ** -126)).sum()), int((tail == 0).sum())))
            assert bool((tail == 0).any())     # expf(-120) is 0 in any float32 arithmetic


SAMPLING = [s for s in GRID if s[1] >= 67 and (s[4] == "underflow" or s[1] == 67)]


@pytest.mark.parametrize("spec", SAMPLING, ids=R.case_id)
def test_heads_act_samples_from_rows_with_zero_entries(spec):
    """act_in == NULL, four seeds: no action is drawn whose returned probability is 0, a row whose returned top probability is 1.0f
    yields `top`, and logp_out is bit for bit what evaluating the drawn action returns."""
    c = R.case_of(spec)
    rows = torch.arange(c.n)
    for seed in (1, 2, 3, 4):
        got = T.run_heads_act(c, None, seed=seed, stream_id=seed + 10)
        a = got["action"].long()
        assert bool(((a >= 0) & (a < c.A)).all())
        assert bool((got["dist"][rows, a] > 0).all()), (seed, int((got["dist"][rows, a] <= 0).sum()))
        sure = got["dist"][rows, c.top] == 1.0
        assert bool((a[sure] == c.top[sure]).all()), seed
        if spec[4] == "underflow":
            assert bool(sure.all()) and bool((got["dist"] == 0).any())
        ev = T.run_heads_act(c, got["action"], outs=("logp",))
        assert torch.equal(ev["logp"].view(torch.int32), got["logp"].view(torch.int32)), seed


# ---- 4. the diagnostics -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [(6, 257, 0, 0, "main", 257), (18, 67, 1, 1, "main", 67)], ids=R.case_id)
def test_heads_diag_on_peaked_policies(spec):
    """ddrl_op_heads_diag: ApproxKL, ClipFraction and RatioMax (and the other sums) against float64 under the tolerances of
    tests/ppo_diag_ref.py; RatioMax reports the 2^20 sample."""
    import ppo_diag_ref as D
    from ddrl4nav_amd import ops
    from test_ppo_diag_gpu import check_against_reference, run_diag
    c = R.case_of(spec)
    got = run_diag(c)
    ref = check_against_reference(c, got, R.case_id(spec))
    want = D.direct_diag(ref["logp"] - c.old_logps.double(), c.rets.double(), ref["value"], c.hyper["ppo_clip"])
    have = ops.diag_dict(got[0])
    assert have["ClipFraction"] == want["ClipFraction"]
    assert abs(have["RatioMax"] - 2.0 ** 20) <= 1e-3 * 2.0 ** 20 and abs(have["RatioMax"] - want["RatioMax"]) <= D.RTOL * want["RatioMax"]
    assert abs(have["ApproxKL"] - want["ApproxKL"]) <= ref["bounds"][1] / c.n + 1e-12 * want["ApproxKL"]


# ---- 5. a policy driven into collapse -------------------------------------------------------------------------------------------------------
def test_operators_stay_finite_while_a_policy_collapses():
    """heads_act (the current log-probabilities as old_logps) -> heads_loss_opt (split entropy bonus, theta 0.01) -> clip + Adam at 1e-2
    on the head arena, 600 times on fixed features: the three statistics and the whole gradient arena of every step are finite, the
    parameters at the end are, and the entropy ends below heads_peaked_ref.H_END (tests/test_heads_peaked_cpu.py: float64 ends 80
    times lower).  Everything stays on the device until the loop is over."""
    _lib, lib = T._load()
    c = R.collapse_case()
    L = H.head_layout(0, c.A)
    d = T._desc(c, L)
    cfg = T._cfg(c, actor_lr=R.COLLAPSE_LR, critic_lr=R.COLLAPSE_LR)
    f = dict(dtype=torch.float32, device="cuda")
    n, npar = c.n, L["n_params"]
    params = H.fill_arena(L, c.params, fill=0.0).cuda()
    grads, m, v = torch.zeros(npar + 8, **f), torch.zeros(npar, **f), torch.zeros(npar, **f)
    wf, wb = c_int64(), c_int64()
    _lib.check(lib.ddrl_op_heads_ws_floats(byref(d), n, byref(wf)))
    _lib.check(lib.ddrl_op_clip_adam_ws_bytes(byref(wb)))
    ws, aws = torch.zeros(wf.value, **f), torch.zeros(wb.value, dtype=torch.uint8, device="cuda")
    ha, hc = c.ha.cuda(), c.hc.cuda()
    acts, adv, ret = (t.contiguous().cuda() for t in (c.actions, c.advs, c.rets))
    dh_a, dh_c = torch.zeros(n, H.FEAT, **f), torch.zeros(n, H.FEAT, **f)
    value, old = torch.zeros(n, **f), torch.zeros(n, **f)
    opt = _lib.LossOptions(0.0, 1)
    steps = R.COLLAPSE_STEPS
    stats, finite = torch.zeros(steps, 3, **f), torch.zeros(steps, dtype=torch.bool, device="cuda")
    p, st = T._p, T._st()
    for t in range(1, steps + 1):
        _lib.check(lib.ddrl_op_heads_act(byref(d), p(params), p(ha), p(hc), n, p(acts), 0, 0, p(None), p(value), p(None), p(old), st))
        _lib.check(lib.ddrl_op_heads_loss_opt(byref(d), byref(cfg), p(params), p(ha), p(hc), n, p(acts), p(old), p(adv), p(ret), byref(opt),
                                              p(None), n, p(dh_a), p(dh_c), p(grads), p(ws), st))
        stats[t - 1] = grads[npar:npar + 3]
        finite[t - 1] = torch.isfinite(grads[:npar + 3]).all() & torch.isfinite(dh_a).all() & torch.isfinite(dh_c).all() & torch.isfinite(old).all()
        _lib.check(lib.ddrl_op_clip_adam(byref(cfg), p(params), p(grads), p(m), p(v), npar, L["critic_w"], 0, t, p(aws), st))
    torch.cuda.synchronize()
    stats, finite = stats.cpu(), finite.cpu()
    ent = stats[:, 2]
    print("entropy: first %.4f, step 6 %.3e, last %.3e; largest of the last hundred %.3e" % (float(ent[0]), float(ent[5]), float(ent[-1]),
                                                                                              float(ent[-100:].max())))
    assert bool(torch.isfinite(stats).all()), "first non-finite statistic at step %d" % (int((~torch.isfinite(stats).all(1)).nonzero()[0]) + 1)
    assert bool(finite.all()), "first non-finite gradient at step %d" % (int((~finite).nonzero()[0]) + 1)
    assert bool(torch.isfinite(params).all()) and bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all())
    assert 1.0 < float(ent[0]) < math.log(c.A)
    assert float(ent[-1]) < R.H_END and float(ent[-100:].max()) < R.H_END


CONTEXT_ITERATIONS, CONTEXT_BATCH = 300, 32
CONTEXT_ACTOR_LR = 2.5e-4          # the actor rate of the run that logged EntLoss = nan


def test_context_stays_finite_while_its_policy_collapses():
    """The whole Atari context, two encoders, loss_options (0.0, True): 300 iterations on 32 fixed frames.  Each iteration samples the
    actions with the acting kernel (so rows with q_j == 0 are sampled from as the policy narrows), rewards action 0 and punishes the
    others, and steps.  Finiteness of the whole gradient arena, its statistics, the sampled log-probabilities and the parameters is
    all that is asserted: the float64 oracle is too slow for 300 network passes."""
    from ddrl4nav_amd.engine import HotPath
    from ddrl4nav_amd.utils.recipe import flatten, make_weights
    B = CONTEXT_BATCH
    rng = np.random.default_rng(41)
    frames = torch.from_numpy(rng.integers(0, 256, size=(B, 4, 84, 84), dtype=np.uint8)).cuda()
    ret = torch.from_numpy(rng.normal(size=B).astype(np.float32)).cuda()
    hp = HotPath(B, n_actions=6, in_channels=4, actor_lr=CONTEXT_ACTOR_LR, ent_loss_theta=0.01)
    try:
        hp.set_params(flatten(make_weights(0)))
        hp.loss_options = (0.0, True)
        one = torch.ones(B, device="cuda")
        finite = torch.zeros(CONTEXT_ITERATIONS, dtype=torch.bool, device="cuda")
        ent = torch.zeros(CONTEXT_ITERATIONS, device="cuda")
        took0 = torch.zeros(CONTEXT_ITERATIONS, device="cuda")
        for it in range(CONTEXT_ITERATIONS):
            probs, value, action, logp = hp.forward(frames, seed=it, stream_id=3)
            adv = torch.where(action == 0, one, -one).contiguous()
            hp._ppo_iter_opt(frames, 0, None, action, logp, adv, ret, None, B, None)
            finite[it] = torch.isfinite(hp.grads).all() & torch.isfinite(logp).all() & torch.isfinite(probs).all() & (probs.gather(1, action.long()[:, None]) > 0).all()
            ent[it] = hp.grads[hp.n_params + 2]
            took0[it] = (action == 0).float().mean()
            hp.clip_adam_step()
            finite[it] &= torch.isfinite(hp.grads[hp.n_params:]).all()
        torch.cuda.synchronize()
        finite, ent, took0 = finite.cpu(), ent.cpu(), took0.cpu()
        print("entropy: %s; share of action 0 at the end %.2f" % (" ".join("%.3e" % float(ent[i]) for i in (0, 50, 100, 150, 200, 250, 299)),
                                                                  float(took0[-1])))
        assert bool(finite.all()), "first non-finite iteration: %d" % int((~finite).nonzero()[0])
        assert bool(torch.isfinite(hp.params).all()) and bool(torch.isfinite(hp.adam_v).all())
    finally:
        hp.close()
