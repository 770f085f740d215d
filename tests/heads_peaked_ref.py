"""What tests/test_heads_peaked_cpu.py and tests/test_heads_peaked_gpu.py share: the grid of peaked cases (heads_ref.make_peaked_case),
the cases that sit ON the closed upper clamp boundary, and the float64 statement of the loop that drives a policy into collapse.
Nothing here needs a GPU."""
import math

import torch

import heads_ref as H
import loss_options_ref as LR

OP_TOL = 2e-5                      # tests/test_heads_optim_ops_gpu.py
SIZES = (2, 6, 8, 18)              # A <= 6, 7..8 and > 8 are the three kernel classes; 2 is the smallest A
BATCHES = (3, 67, 257)


def grid():
    """(A, n, shared, smooth, kind, B_global): every A x n once with the main gaps, sharing mode, value loss and B_global spread over them
    (each A meets both sharing modes and both value losses), and per A two class (e) cases ("underflow": gaps 95 and 120 only)."""
    cases = []
    for i, A in enumerate(SIZES):
        for j, n in enumerate(BATCHES):
            cases.append((A, n, (i + j) % 2, ((i + j) // 2 + j) % 2, "main", n if (i + j) % 2 else 3 * n + 1))
    for i, A in enumerate(SIZES):
        cases.append((A, 67, i % 2, (i // 2) % 2, "underflow", 67))
        cases.append((A, 257, 1 - i % 2, 1 - (i // 2) % 2, "underflow", 772))
    return cases


def opt_grid():
    """(A, n, shared, smooth, kind, B_global, option set): the option sets `entropy` and `both` of loss_options_ref, split encoders above
    all (entropy_split does nothing with a shared one), two shared cases for the clipped value loss on peaked rows."""
    cases = []
    for i, A in enumerate(SIZES):
        cases.append((A, 67, 0, i % 2, "main", 67, "entropy"))
        cases.append((A, 257, 0, 1 - i % 2, "main", 772, "both"))
        cases.append((A, 67, 0, (i // 2) % 2, "underflow", 202, "both" if i % 2 else "entropy"))
    cases += [(6, 3, 0, 0, "main", 3, "entropy"), (6, 67, 1, 0, "main", 67, "both"), (18, 3, 1, 1, "main", 10, "entropy")]
    return cases


def case_of(spec):
    A, n, shared, smooth, kind, B = spec[:6]
    c = H.make_peaked_case(A, n, shared, smooth, seed=1, B_global=B, gaps=H.UNDERFLOW_GAPS if kind == "underflow" else None)
    if len(spec) > 6:
        LR.attach_options(c, LR.OPTION_SETS[spec[6]])
    return c


def case_id(spec):
    A, n, shared, smooth, kind, B = spec[:6]
    return "cat%d-n%d-%s-%s-%s-B%d%s" % (A, n, "shared" if shared else "split", "huber" if smooth else "mse", kind, B,
                                         "-" + spec[6] if len(spec) > 6 else "")


def row_tol(c):
    return H.peaked_row_tol(c, OP_TOL)


def entropy_mass(c):
    """Per row, the magnitude of what cancels inside the entropy term's share of d(loss)/d(h_actor): d(-theta H)/d(z_j) is
    q_j (g_j - sum_k q_k g_k) with g_j = theta / B (lc_j + [q_j in range]) -- at a uniform row the differences vanish altogether, at a
    saturated one q_top g_top (1e-7) stands against a result of 1e-17 -- times the largest actor weight (1: the control columns).  Zero
    where the entropy is not differentiated (split encoders without the option)."""
    if not (c.shared or getattr(c, "entropy_split", False)):
        return torch.zeros(c.n, dtype=torch.float64)
    q = torch.softmax(c.z64, dim=-1)
    inr = ((q >= H.CAT_EPS) & (q <= 1.0 - H.CAT_EPS)).double()
    lc = torch.log(torch.clamp(q, H.CAT_EPS, 1.0 - H.CAT_EPS))
    terms = (q * (lc + inr).abs()).amax(1)
    return c.hyper["ent_loss_theta"] / float(c.B_global) * terms * float(c.params["actor_w"].abs().max())


# ---- ON the closed upper boundary ---------------------------------------------------------------------------------------------------------
# torch.clamp passes the gradient on the CLOSED interval, and 1 - eps is a float32 number.  The peaked recipe keeps away from it (a tail
# within a factor of three of eps may round onto it, and float32 and float64 then sit on different sides); these rows go there on
# purpose, from the side on which both agree: one tail action at -BOUNDARY_GAP, every other at -60, so the tail sum is t = 1.125 eps in
# float64 -- q_top = 1 - 1.125 eps, inside the interval -- and float32 has s = fl(1 + t) = 1 + eps, p_top = fl(1 / (1 + eps)) = 1 - eps,
# sum(p) = fl(1 + 0.125 eps) = 1: q_top = 1 - eps EXACTLY, whatever the last bits of t (|logit error| ~1e-5 against a window of
# 0.75 eps < t < 1.25 eps).  A kernel that closes the interval passes the gradient, as float64 does; one that opens it returns zeros.
BOUNDARY_GAP = -math.log(1.125 * H.CAT_EPS)
# What a float32 evaluation may lose on such a row: it holds q_top as 1 - eps where float64 has 1 - t, so a term formed as (1 - q_top)
# is off by the factor eps / t = 1 / 1.125 (the kernels form it as the sum of the other p_j and lose nothing: measured 0.0000).  Actor gradient of a row that took `top` -- g (1 - q_top) -- 11 % low: bound 0.2.  Entropy gradient
# with a zero advantage -- q_j (g_j - sum_k q_k g_k), g_j = -(lc_j + 1) inside the interval: the misheld term is 1 of |lc_tail + 1| =
# 14.8, under 1 % in all -- bound 0.03; opening the interval at the top drops the `+ 1` of the top action and moves the row by 6 %.
BOUNDARY_ACTOR_TOL, BOUNDARY_ENTROPY_TOL = 0.2, 0.03


def make_boundary_case(A, n, shared, seed=3):
    """Every row on the boundary.  Rows b % 2 == 0 took `top` under a solid advantage at ratio 1 (the surrogate passes its gradient to the
    log-probability); the others have advantage exactly 0 (only the entropy term reaches the logits)."""
    c = H.make_case(0, A, n, shared, 0, seed=seed)
    g = torch.Generator().manual_seed(4242 + 31 * A + n)
    K = H.control_columns(A)
    c.params["actor_w"][:, K] = torch.eye(A)
    c.params["critic_w"][K] = 0.0
    c.top = torch.randint(0, A, (n,), generator=g)
    c.tail = (c.top + 1 + torch.randint(0, A - 1, (n,), generator=g)) % A
    target = torch.full((n, A), -60.0, dtype=torch.float64)
    target[torch.arange(n), c.tail] = -BOUNDARY_GAP
    target[torch.arange(n), c.top] = 0.0
    ha64 = c.ha.double()
    ha64[:, K] = 0.0
    z0 = ha64 @ c.params["actor_w"].double().T + c.params["actor_b"].double()
    c.ha[:, K] = (target - z0).float()
    c.actions = c.top.float()
    took = torch.arange(n) % 2 == 0
    sign = torch.where(torch.arange(n) % 4 == 0, 1.0, -1.0).double()
    H._place(c, g, sign, torch.ones(n, dtype=torch.float64))
    c.advs = torch.where(took, torch.where(c.advs.abs() < 0.1, sign.float(), c.advs), torch.zeros(n))
    c.took = took
    P64 = {k: v.double() for k, v in c.params.items()}
    c.z64 = c.ha.double() @ P64["actor_w"].T + P64["actor_b"]
    c.outcomes = [H.outcome_of(float(c.advs[i]), float(c.r64[i]), c.hyper) for i in range(n)]
    return c


def check_boundary_case(c):
    """float64 is inside the interval with the tail in the window; torch's own float32 forward has q_top == 1 - eps to the bit."""
    q = torch.softmax(c.z64, dim=-1)
    not_top = torch.ones(c.n, c.A, dtype=torch.bool)
    not_top[torch.arange(c.n), c.top] = False
    tail = (q * not_top).sum(1)      # summed directly, not 1 - q_top
    assert bool(((tail > 1.05 * H.CAT_EPS) & (tail < 1.2 * H.CAT_EPS)).all()), (float(tail.min() / H.CAT_EPS), float(tail.max() / H.CAT_EPS))
    P32 = {k: v.float() for k, v in c.params.items()}
    probs32 = H.forward(c, c.ha, c.ha if c.shared else c.hc, P32, torch.float32)[0]
    q32 = probs32 / probs32.sum(-1, keepdim=True)
    assert bool((q32[torch.arange(c.n), c.top] == torch.tensor(1.0 - H.CAT_EPS, dtype=torch.float32)).all())
    assert bool((c.r64[c.took] - 1.0).abs().max() < 1e-5) and bool((c.advs[c.took].abs() >= 0.1).all()) and bool((c.advs[~c.took] == 0).all())


# ---- a policy driven into collapse --------------------------------------------------------------------------------------------------------
COLLAPSE_A, COLLAPSE_N, COLLAPSE_STEPS, COLLAPSE_LR = 6, 64, 600, 1e-2
COLLAPSE_HYPER = dict(H.DEFAULT_HYPER, ent_loss_theta=0.01)
FAVOURED = 0
# Mean entropy after the 600 steps.  The float64 loop below falls from 1.47 (log 6 = 1.79) to 1.5e-7 within six steps and ends at 1.19e-7 =
# -log(1 - eps), the floor of the clamped entropy: every row saturated, the logit gaps near 50 -- Adam's momentum carries them far past
# the clamps that have shut both gradients off.  float32 and float64 take different paths there (Adam divides by the root of a running
# square: a last-place difference in a vanishing gradient is a different step), so the end points are not compared; the threshold only
# says "collapsed", 80 times above where float64 ends.
H_END = 1e-5


def collapse_case():
    """Split encoders, option set `entropy` with ent_loss_theta 0.01: fixed features -- one common direction plus per-sample noise, as
    the states of one game are, so that what a row learns moves every row -- uniform actions, an advantage of +|a| where the action is
    FAVOURED and -|a| elsewhere, returns a unit normal.  old_logps is refilled each step with the current policy's log-probabilities
    (ratio 1: a fixed column would let the clip stop the policy after a few steps)."""
    c = H.make_case(0, COLLAPSE_A, COLLAPSE_N, 0, 0, COLLAPSE_HYPER, seed=6)
    g = torch.Generator().manual_seed(99)
    c.ha = 0.5 * torch.randn(1, H.FEAT, generator=g) + 0.2 * torch.randn(COLLAPSE_N, H.FEAT, generator=g)
    c.actions = torch.randint(0, COLLAPSE_A, (COLLAPSE_N,), generator=g).float()
    mag = 0.5 + torch.rand(COLLAPSE_N, generator=g)
    c.advs = torch.where(c.actions == FAVOURED, mag, -mag)
    c.rets = torch.randn(COLLAPSE_N, generator=g)
    LR.attach_options(c, LR.OPTION_SETS["entropy"])
    return c


def adam_settings():
    from ddrl4nav_amd import _lib
    cfg = _lib.default_config()
    f = lambda x: float(torch.tensor(x, dtype=torch.float32))
    return dict(beta1=f(cfg.adam_beta1), beta2=f(cfg.adam_beta2), eps=f(cfg.adam_eps), max_norm=f(cfg.clip_grad_norm), clip=bool(cfg.clip_grad))


def collapse_loop64(c, steps=COLLAPSE_STEPS, lr=COLLAPSE_LR):
    """The loop of the GPU test in float64 torch: loss block with the options (loss_options_ref.loss_block), clip_grad_norm_ + Adam on the
    four head tensors (heads_ref.clip_coef64 / adam64).  Returns the [steps, 3] loss shares and the final parameters."""
    s = adam_settings()
    names = ("actor_w", "actor_b", "critic_w", "critic_b")
    c.params = {k: v.double().clone() for k, v in c.params.items()}
    shapes = [c.params[k].shape for k in names]
    m = torch.zeros(sum(int(torch.tensor(sh).prod()) for sh in shapes), dtype=torch.float64)
    v = m.clone()
    lr_t = torch.full_like(m, lr)
    stats = []
    for t in range(1, steps + 1):
        ha = c.ha.double()
        c.old_logps = H.forward(c, ha, c.hc.double(), c.params, torch.float64)[1]
        r = LR.loss_block(c, torch.float64)
        stats.append(r["losses"])
        gflat = torch.cat([r["g_" + k].reshape(-1) for k in names])
        assert bool(torch.isfinite(gflat).all()), t
        _, coef = H.clip_coef64(gflat, s["max_norm"], s["clip"])
        p = torch.cat([c.params[k].reshape(-1) for k in names])
        upd, m, v, _ = H.adam64(p, gflat, m, v, lr_t, t, s["beta1"], s["beta2"], s["eps"], coef)
        p = p + upd
        o = 0
        for k, sh in zip(names, shapes):
            cnt = c.params[k].numel()
            c.params[k] = p[o:o + cnt].reshape(sh)
            o += cnt
    return torch.stack(stats), c.params
