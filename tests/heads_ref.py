"""Shared pieces of tests/test_heads_optim_ops_gpu.py: the input recipe that reaches every branch of the PPO loss block, a
plain torch restatement of that block (run in float64 as the reference and in float32 as the yardstick), float64
restatements of clip_grad_norm_ + Adam / RMSprop, and the arena layout the head kernels are driven with.  Nothing here
needs a GPU.

The loss expressions are those of tests/golden/make_golden.py (F3) and oracle/ddrl_oracle.py:ppo_losses /
oracle/ddrl_oracle_nav.py:losses, applied to GIVEN 512-wide features instead of an encoder's output."""
import math

import numpy as np
import torch

FEAT = 512
CAT_EPS = 2.0 ** -23           # torch.finfo(float32).eps: include/ddrl.h defines logp = log(clamp(p_hat, eps, 1 - eps)) with it
FLOOR = 2.0 ** -25             # mean error (relative to the largest element) of a correctly rounded fp32 tensor: no yardstick below it

DEFAULT_HYPER = dict(ppo_clip=0.2, dual_clip=3.0, v_loss_theta=1.0, ent_loss_theta=0.05)
OTHER_HYPER = dict(ppo_clip=0.1, dual_clip=2.0, v_loss_theta=0.5, ent_loss_theta=0.01)
# target ratios: every one at least 0.1 from 1 - clip, 1 + clip and dual_clip of its hyper-parameter set
RATIOS = {0.2: (0.5, 0.7, 0.9, 1.0, 1.1, 1.5, 2.5, 3.5, 6.0), 0.1: (0.5, 0.7, 0.78, 1.0, 1.22, 1.5, 1.8, 2.5, 6.0)}
HUBER_E = (-3.0, -1.5, -0.5, 0.0, 0.5, 1.5, 3.0)

OUTCOMES = ("pos_below", "pos_inside", "pos_above", "neg_below", "neg_inside", "neg_between", "neg_dual", "zero")
# the fixed subset of a batch too small to hold all of them: sample 0 takes the dual-clip branch, 1 an unclipped positive one, 2 the
# stretch between 1 + clip and dual_clip
SMALL_N_OUTCOMES = {1: ("neg_dual",), 3: ("neg_dual", "pos_inside", "neg_between")}


def _pairs(ratios):
    """(sign of adv, target ratio) in the order the samples cycle through: all 18 pairs, the rare branches first."""
    lo_hi = [r for r in ratios]
    dual_r, between_r = lo_hi[-2], lo_hi[-3]
    first = [(-1, dual_r), (+1, 1.0), (-1, between_r), (+1, lo_hi[0]), (-1, lo_hi[2]), (+1, lo_hi[5])]
    rest = [(s, r) for r in ratios for s in (+1, -1) if (s, r) not in first]
    return first + rest


def outcome_of(adv, r, hyper):
    """Which of the eight outcomes of ppo_surrogate (csrc/ppo_math.h) a sample with advantage adv and ratio r takes."""
    lo, hi, dual = 1.0 - hyper["ppo_clip"], 1.0 + hyper["ppo_clip"], hyper["dual_clip"]
    if adv == 0:
        return "zero"
    if adv > 0:
        return "pos_below" if r < lo else ("pos_inside" if r <= hi else "pos_above")
    if r < lo:
        return "neg_below"
    if r <= hi:
        return "neg_inside"
    return "neg_between" if r < dual else "neg_dual"


class Case:
    pass


def head_params(continuous, A, g):
    p = {"actor_w": torch.randn(A, FEAT, generator=g) * 0.05, "actor_b": torch.randn(A, generator=g) * 0.1,
         "critic_w": torch.randn(FEAT, generator=g) * 0.05, "critic_b": torch.randn(1, generator=g) * 0.1}
    if continuous:
        p["log_std"] = torch.rand(A, generator=g) * 1.5 - 1.0
    return p


def forward(c, ha, hc, P, dtype):
    """dist (probs / mu), log-prob of c.actions, per-sample entropy, value -- plain torch in `dtype`."""
    z = ha @ P["actor_w"].T + P["actor_b"]
    v = hc @ P["critic_w"] + P["critic_b"]
    if c.continuous:
        std = torch.exp(P["log_std"])
        pi = torch.distributions.Normal(z, std)
        return z, pi.log_prob(c.actions.to(dtype)).sum(-1), pi.entropy().mean(-1), v, z
    probs = torch.softmax(z, dim=-1)
    p_hat = probs / probs.sum(-1, keepdim=True)
    lc = torch.log(torch.clamp(p_hat, CAT_EPS, 1.0 - CAT_EPS))
    logp = lc.gather(1, c.actions.long()[:, None])[:, 0]
    return probs, logp, -(lc * p_hat).sum(-1), v, z


def make_case(continuous, A, n, shared, smooth, hyper=None, seed=0, B_global=None):
    """The deterministic input recipe: features N(0, 1) x 0.5, head weights N(0, 0.05), biases N(0, 0.1), log_std U[-1, 0.5];
    old_logps placed so that the ratio of sample i is the i-th target of the cycle, advantages of both signs (one in ten
    1e-4 of the rest, every 16th exactly 0), returns at the cycle of distances HUBER_E from the value."""
    hyper = dict(hyper or DEFAULT_HYPER)
    g = torch.Generator().manual_seed(1000 * seed + 37 * A + n + (500 if continuous else 0))
    c = Case()
    c.continuous, c.A, c.n, c.shared, c.smooth, c.hyper = bool(continuous), A, n, bool(shared), bool(smooth), hyper
    c.B_global = n if B_global is None else B_global
    c.params = head_params(continuous, A, g)
    c.ha = torch.randn(n, FEAT, generator=g) * 0.5
    c.hc = torch.randn(n, FEAT, generator=g) * 0.5       # shared: a DIFFERENT finite buffer that must not be read
    P64 = {k: v.double() for k, v in c.params.items()}
    ha64 = c.ha.double()
    hc64 = ha64 if shared else c.hc.double()
    if continuous:
        mu64 = ha64 @ P64["actor_w"].T + P64["actor_b"]
        c.actions = (mu64 + torch.exp(P64["log_std"]) * torch.randn(n, A, generator=g).double()).float()
    else:
        a = torch.arange(n) % A                          # every action present (n >= A), in a shuffled order
        c.actions = a[torch.randperm(n, generator=g)].float()
    pairs = _pairs(RATIOS[round(hyper["ppo_clip"], 3)])
    sign = torch.tensor([pairs[i % 18][0] for i in range(n)], dtype=torch.float64)
    target = torch.tensor([pairs[i % 18][1] for i in range(n)], dtype=torch.float64)
    _place(c, g, sign, target)
    return c


def _place(c, g, sign, target):
    """The batch columns that depend on the policy, placed from the float64 forward of the case's features, parameters and actions:
    advantages of the given signs, old_logps for the target ratios, returns at the Huber cycle of distances from the value."""
    n, hyper = c.n, c.hyper
    P64 = {k: v.double() for k, v in c.params.items()}
    ha64 = c.ha.double()
    hc64 = ha64 if c.shared else c.hc.double()
    _, logp64, _, v64, _ = forward(c, ha64, hc64, P64, torch.float64)
    idx = torch.arange(n)
    mag = torch.randn(n, generator=g).double().abs() * torch.where(idx % 10 == 7, 1e-4, 1.0)
    adv = sign * mag
    if n >= 16:
        adv[idx % 16 == 15] = 0.0
    c.advs = adv.float()
    c.old_logps = (logp64 - torch.log(target)).float()
    e = torch.tensor([HUBER_E[i % 7] for i in range(n)], dtype=torch.float64)
    c.rets = (v64 + e * (1.0 + 0.05 * (2.0 * torch.rand(n, generator=g).double() - 1.0))).float()
    # what the float64 reference really sees after the inputs were rounded to float32
    c.r64 = torch.exp(logp64 - c.old_logps.double())
    c.err64 = c.rets.double() - v64
    c.logp64 = logp64
    c.outcomes = [outcome_of(float(c.advs[i]), float(c.r64[i]), hyper) for i in range(n)]
    return c


def check_recipe(c, every_action=True):
    """The recipe's own promises (a CPU test runs them for every case of the GPU grid): every sample's float64 ratio sits
    more than 1e-3 from each branch boundary, so the fp32 ratio a kernel forms (|log-prob error| ~1e-6) lands in the same
    branch; the batch holds every outcome (a fixed subset below 64 samples); with the Huber loss all three pieces of its
    gradient occur and no |err| is within 1e-3 of 1.  every_action = False: the batch need not hold every action (the
    peaked recipe below draws them at random)."""
    h = c.hyper
    bounds = torch.tensor([1.0 - h["ppo_clip"], 1.0 + h["ppo_clip"], h["dual_clip"]], dtype=torch.float64)
    margin = (c.r64[:, None] - bounds[None, :]).abs().min().item()
    assert margin > 1e-3, margin
    assert torch.isfinite(c.old_logps).all() and torch.isfinite(c.rets).all()
    have = set(c.outcomes)
    want = set(OUTCOMES) if c.n >= 64 else set(SMALL_N_OUTCOMES.get(c.n, ()))
    assert want <= have, sorted(want - have)
    if c.n >= 64:
        faint = (c.advs != 0) & (c.advs.abs() < 1e-3)
        assert faint.any() and (c.advs.abs() > 1e-2).any()
        if not c.continuous and every_action:
            assert set(int(a) for a in c.actions) == set(range(c.A))
    ae = c.err64.abs()
    assert ((ae - 1.0).abs() > 1e-3).all(), float((ae - 1.0).abs().min())
    if c.n >= 7:
        assert (c.err64 > 1.0).any() and (c.err64 < -1.0).any() and ((ae < 1.0) & (ae > 0.1)).any() and (ae < 1e-5).any()


# ---- peaked and collapsed policies ------------------------------------------------------------------------------------------------------
# make_case draws logits with a standard deviation of about 0.6: every policy is close to uniform and no q_j comes near a clamp of
# log(clamp(q, eps, 1 - eps)).  The recipe below PLACES the logits: one `top` action at 0, the others at -gap, so that every clamp, the
# subnormal range of expf and its underflow are met at a stated distance.
LOG_EPS = math.log(CAT_EPS)
FAR_RATIOS = (2.0 ** 20, 2.0 ** -20, 2.0 ** 10, 2.0 ** -10)
ENTRY_MARGIN = 0.05      # |log q_j - log eps| of every entry: fp32 logits are off by ~1e-5 at most, 5,000 times less
TAIL_MARGIN = 1.5        # |log(sum_{j != top} q_j) - log eps|: below 1 the fp32 spacing is 2^-24 = eps / 2, so q_top = 1 - tail is resolved
                         # to a QUARTER of eps and 1 - eps itself is a number: a tail within a factor of ~3 of eps can round onto the closed
                         # boundary (flips seen at a log-margin of 0.29, none from 0.69 up)
UNDERFLOW_GAPS = (95.0, 120.0)    # class (e): expf(-95) = 5.5e-42 is an fp32 subnormal, expf(-120) is 0


def peaked_gaps(A):
    """The gaps the samples cycle through, rare classes first (a batch of three holds a saturated, a peaked and -- A >= 8 -- a class (c)
    row).  Classes: (a) near uniform: 0, 3; (b) peaked, every clamp in range: 9, 13 (and 14.25 for A = 2); (c) every tail entry below
    eps while the top is still below 1 - eps: needs e^-gap < eps e^-ENTRY_MARGIN and (A - 1) e^-gap > eps e^TAIL_MARGIN, that is
    15.99 < gap < 15.94 + log(A - 1) - 1.5, empty below A = 8 (log 7 = 1.95) -- 16.2 for A >= 8, left out for smaller A; (d) both
    saturated: 20.5, 30, 40.  A = 2 cannot take 16.2 at all: its one tail entry would sit 0.26 from eps."""
    if A == 2:
        return (20.5, 13.0, 0.0, 40.0, 9.0, 3.0, 30.0, 14.25)
    if A < 8:
        return (20.5, 13.0, 0.0, 40.0, 9.0, 3.0, 30.0)
    return (20.5, 13.0, 16.2, 0.0, 40.0, 9.0, 3.0, 30.0)


def control_columns(A):
    """One feature column per action, reserved to steer its logit."""
    return [7 + 29 * j for j in range(A)]


def make_peaked_case(A, n, shared, smooth, hyper=None, seed=0, B_global=None, gaps=None):
    """make_case(0, ...) with PLACED logits.  Features, weights, advantages and returns stay dense and random; actor_w[:, K] = I and
    critic_w[K] = 0 on the control columns K, and ha[b, K_j] = target[b, j] - z0[b, j] formed in float64 (z0: the logits without the
    control features), so the float64 logits are the targets up to the fp32 rounding of that one feature and the fp32 logits differ from
    them by dot-product rounding only.  Target of sample b: `top` at 0, the other actions at -gap_b, plus one shift per sample from
    U[-1, 1].  gap_b cycles through `gaps` (default peaked_gaps(A); UNDERFLOW_GAPS is class (e), kept in cases of its own because its rows
    carry a wider tolerance, peaked_row_tol).  Every third sample takes `top`, the others a uniform action -- tail actions with
    q < eps included.  Ratios: the 18-pair cycle of make_case, but every ninth sample takes a far ratio 2^+-20, 2^+-10 with alternating
    sign of the advantage instead -- never where the advantage is exactly 0 (inf * 0 is torch's answer there too)."""
    c = make_case(0, A, n, shared, smooth, hyper, seed=seed, B_global=B_global)
    g = torch.Generator().manual_seed(7919 * seed + 37 * A + n + 1)
    gaps = tuple(peaked_gaps(A) if gaps is None else gaps)
    L = len(gaps)
    K = control_columns(A)
    c.params["actor_w"][:, K] = torch.eye(A)
    c.params["critic_w"][K] = 0.0
    c.gaps = gaps
    c.gap = torch.tensor([gaps[(b + b // L) % L] for b in range(n)], dtype=torch.float64)     # one step more per round: no lock-step with the other cycles
    c.top = torch.randint(0, A, (n,), generator=g)
    shift = 2.0 * torch.rand(n, generator=g).double() - 1.0
    target = -c.gap[:, None].repeat(1, A)
    target[torch.arange(n), c.top] = 0.0
    target = target + shift[:, None]
    ha64 = c.ha.double()
    ha64[:, K] = 0.0
    z0 = ha64 @ c.params["actor_w"].double().T + c.params["actor_b"].double()
    c.ha[:, K] = (target - z0).float()
    uniform = torch.randint(0, A, (n,), generator=g)
    c.actions = torch.where(torch.arange(n) % 3 == 0, c.top, uniform).float()
    pairs = _pairs(RATIOS[round(c.hyper["ppo_clip"], 3)])
    sign = [float(pairs[i % 18][0]) for i in range(n)]
    ratio = [float(pairs[i % 18][1]) for i in range(n)]
    k = 0
    c.far = torch.zeros(n, dtype=torch.bool)
    for i in range(n):
        if i % 9 == 4 and not (n >= 16 and i % 16 == 15):
            sign[i], ratio[i] = (1.0, -1.0)[k % 2], FAR_RATIOS[(k // 2) % 4]
            c.far[i] = True
            k += 1
    _place(c, g, torch.tensor(sign, dtype=torch.float64), torch.tensor(ratio, dtype=torch.float64))
    P64 = {k_: v.double() for k_, v in c.params.items()}
    c.z64 = c.ha.double() @ P64["actor_w"].T + P64["actor_b"]
    return c


def ulp32(x):
    """Spacing of float32 at |x| (float64 tensor in, float64 out)."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


def peaked_row_tol(c, base):
    """Per-row tolerance of a peaked case: a row's relative gradient error is about the ABSOLUTE error of its logit gaps, and the last
    roundings of a logit -- the six levels of a 64-lane butterfly plus the bias add, half an ulp each, for the two logits of a gap -- happen
    at magnitude max_j |z_bj|: base + 8 ulp32(max_j |z_bj|).  Within 10 % of `base` = 2e-5 for |z| < 4, 5e-5 at |z| = 41, 8e-5 at 121."""
    return base + 8.0 * ulp32(c.z64.abs().amax(1))


def check_peaked_recipe(c):
    """The peaked recipe's promises, in float64 (a CPU test runs them for every case of the GPU grid): every entry's log q_j more than
    ENTRY_MARGIN from log eps; every row's log tail sum (summed directly, not 1 - q_top) more than TAIL_MARGIN from log eps; torch's own
    fp32 forward puts every q_j < eps and q_j > 1 - eps comparison on the side float64 puts it; the ratio and Huber margins of
    check_recipe; from 64 samples up all eight outcomes of the surrogate, far ratios of both directions under advantages of both signs
    (all four far ratios from 257 up), a taken action with q < eps and one with q > 1 - eps -- or, in a class (e) case, a tail entry
    that is a positive fp32 subnormal after exp and one that is exactly 0."""
    check_recipe(c, every_action=False)
    n, A = c.n, c.A
    logq = torch.log_softmax(c.z64, dim=-1)
    q = torch.exp(logq)
    entry = float((logq - LOG_EPS).abs().min())
    assert entry > ENTRY_MARGIN, entry
    not_top = torch.ones(n, A, dtype=torch.bool)
    not_top[torch.arange(n), c.top] = False
    tail = (q * not_top).sum(1)
    tmargin = float((torch.log(tail) - LOG_EPS).abs().min())
    assert tmargin > TAIL_MARGIN, tmargin
    P32 = {k: v.float() for k, v in c.params.items()}
    probs32, _, _, _, z32 = forward(c, c.ha, c.ha if c.shared else c.hc, P32, torch.float32)
    q32 = probs32 / probs32.sum(-1, keepdim=True)
    eps32 = torch.tensor(CAT_EPS, dtype=torch.float32)
    assert torch.equal(q32 < eps32, q < CAT_EPS), "fp32 crosses the lower clamp"
    assert torch.equal(q32 > 1.0 - eps32, q > 1.0 - CAT_EPS), "fp32 crosses the upper clamp"
    assert not bool(((c.advs == 0) & c.far).any())
    qa = q.gather(1, c.actions.long()[:, None])[:, 0]
    e32 = torch.exp(z32 - z32.amax(1, keepdim=True))
    underflow = set(c.gaps) <= set(UNDERFLOW_GAPS)
    if underflow:
        assert bool((c.z64.abs().amax(1) > 90.0).all())
    if n < 64:
        return
    assert set(c.outcomes) == set(OUTCOMES)
    far = c.r64[c.far]
    adv = c.advs[c.far]
    for want in FAR_RATIOS[:2] if n < 257 else FAR_RATIOS:
        hit = (far / want - 1.0).abs() < 1e-3
        assert bool((hit & (adv > 0)).any()) and bool((hit & (adv < 0)).any()), want
    assert bool((qa < CAT_EPS).any()) and bool((qa > 1.0 - CAT_EPS).any())
    if underflow:
        assert bool(((e32 > 0) & (e32 < 2.0 ** -126)).any()) and bool((e32 == 0).any())
    else:
        have = set(float(x) for x in c.gap)
        assert have == set(c.gaps), sorted(set(c.gaps) - have)


def loss_block(c, dtype):
    """The loss block of PPO.learn and its autograd backward on the case's inputs, everything in `dtype` and scaled by
    n / B_global.  Non-shared: actor_loss.backward() and v_loss.backward(); shared: one backward of
    actor_loss + v_theta * v_loss - ent_theta * entropy."""
    h = c.hyper
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in c.params.items()}
    ha = c.ha.to(dtype).clone().requires_grad_(True)
    hc = ha if c.shared else c.hc.to(dtype).clone().requires_grad_(True)
    dist, logp, ent_el, v, _ = forward(c, ha, hc, P, dtype)
    adv, old, ret = c.advs.to(dtype), c.old_logps.to(dtype), c.rets.to(dtype)
    ratio = torch.exp(logp - old)
    m = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - h["ppo_clip"], 1.0 + h["ppo_clip"]) * adv)
    term = torch.where(adv > 0, m, torch.max(m, h["dual_clip"] * adv))
    if c.smooth:   # F.smooth_l1_loss(ret, v), beta = 1, written out
        ae = (ret - v).abs()
        v_el = torch.where(ae < 1.0, 0.5 * (ret - v) ** 2, ae - 0.5)
    else:
        v_el = (ret - v) ** 2 / 2
    s = c.n / float(c.B_global)
    actor_loss, v_loss, ent = -term.mean() * s, v_el.mean() * s, ent_el.mean() * s
    if c.shared:
        (actor_loss + h["v_loss_theta"] * v_loss - h["ent_loss_theta"] * ent).backward()
    else:
        actor_loss.backward(retain_graph=True)
        v_loss.backward()
    out = {"dist": dist.detach(), "logp": logp.detach(), "value": v.detach(), "dh_actor": ha.grad,
           "dh_critic": None if c.shared else hc.grad,
           "losses": torch.stack([actor_loss, v_loss, ent]).detach()}
    for k, p in P.items():
        out["g_" + k] = p.grad
    return {k: (None if t is None else t.detach().double()) for k, t in out.items()}


# ---- arena layout ---------------------------------------------------------------------------------------------------------------
def head_layout(continuous, A):
    """Offsets (in floats) of the head parameters inside a flat arena, the loosest placement the kernels take.  What
    csrc/heads.hip and csrc/gheads.hip need: the categorical kernels with A <= 8 read the actor weight rows with 16-byte
    loads (load_head_weights, register variant), so actor_w is a multiple of 4 floats there; every other slot -- the
    Gaussian head's and the A > 8 actor weights, both biases, log_std, the critic weights -- is read with 4-byte loads and
    sits at an offset that is NOT a multiple of 4."""
    def odd(o):
        return o + 1 if o % 4 == 0 else o
    L = {}
    o = 8 if (not continuous and A <= 8) else 5
    L["actor_w"] = o
    o = odd(o + A * FEAT + 1)
    L["actor_b"] = o
    o = odd(o + A + 2)
    L["log_std"] = o if continuous else 0
    if continuous:
        o = odd(o + A + 1)
    L["critic_w"] = o
    o = odd(o + FEAT + 3)
    L["critic_b"] = o
    L["n_params"] = o + 1 + 6
    L["slots"] = [(L["actor_w"], A * FEAT, "actor_w"), (L["actor_b"], A, "actor_b"), (L["critic_w"], FEAT, "critic_w"),
                  (L["critic_b"], 1, "critic_b")] + ([(L["log_std"], A, "log_std")] if continuous else [])
    return L


def fill_arena(L, params, fill=0.0):
    arena = torch.full((L["n_params"],), float(fill))
    for off, cnt, name in L["slots"]:
        arena[off:off + cnt] = params[name].reshape(-1)
    return arena


# ---- optimiser steps ---------------------------------------------------------------------------------------------------------------
def clip_coef64(g64, max_norm, clip=True):
    """torch.nn.utils.clip_grad_norm_: (norm, coefficient) of a float64 gradient."""
    norm = float(torch.sqrt((g64 * g64).sum()))
    coef = min(max_norm / (norm + 1e-6), 1.0) if clip else 1.0
    return norm, coef


def adam64(p, g, m, v, lr, step, beta1, beta2, eps, coef):
    """One torch.optim.Adam step in float64 on the clipped gradient; lr: per-element tensor.  -> (update, m, v, g clipped)"""
    g = g * coef
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = torch.sqrt(v) / math.sqrt(bc2) + eps
    return -(lr / bc1) * (m / denom), m, v, g


def rmsprop64(g, sq, lr, alpha, eps, coef):
    g = g * coef
    sq = sq * alpha + (1.0 - alpha) * g * g
    return -lr * g / (torch.sqrt(sq) + eps), sq, g


def optim_inputs(n, seed, grad_kind, step):
    """params (half of them exactly 0, so that the update is seen without the rounding of p + update), gradients spanning
    1e-8 .. 1e2 in magnitude, first / second moments as after `step - 1` steps (v non-negative, some exactly 0)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * 0.05
    p[torch.arange(n) % 2 == 0] = 0.0
    grad = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 10.0 - 8.0)
    if grad_kind == "small":       # norm below the clip threshold
        grad = grad * (0.1 / max(float(grad.double().norm()), 1e-30))
    elif grad_kind == "big":       # far above it
        grad = grad * (50.0 / max(float(grad.double().norm()), 1e-30))
    elif grad_kind == "zero":
        grad = torch.zeros(n)
    if step > 1:
        m = torch.randn(n, generator=g) * grad.abs().clamp_min(1e-8)
        v = (torch.randn(n, generator=g) * grad).pow(2)
        v[torch.arange(n) % 5 == 3] = 0.0
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, grad, m, v
