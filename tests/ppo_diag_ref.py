"""Shared pieces of tests/test_ppo_diag_cpu.py and tests/test_ppo_diag_gpu.py: the operator-level case grid of the diagnostics head
(ddrl_op_heads_diag), its float64 reference on the cases of tests/heads_ref.py, and the tolerances of the eight sums propagated
from what the project states for a log-prob and a value (rtol 1e-5, atol 1e-6).  Nothing here needs a GPU."""
import math

import torch

import heads_ref as H

NS = (1, 3, 4, 5, 33, 257, 1025)       # the edges of "four samples per wave turn, four waves per workgroup", more than one workgroup
RTOL, ATOL = 1e-5, 1e-6

# (continuous, A, shared, critic_below): every size with both head arrangements; the negative actor -> critic stride once
GRID = [(0, A, sh, False) for A in (2, 6, 18) for sh in (False, True)] + [(0, 6, False, True)] + \
       [(1, D, sh, False) for D in (1, 2, 8) for sh in (False, True)]


def case_id(cont, A, shared, below):
    return "%s%d_%s%s" % ("gauss" if cont else "cat", A, "shared" if shared else "split", "_below" if below else "")


def make_case(cont, A, n, shared, rets=None):
    """heads_ref.make_case (n < A included: the actions are a shuffle of arange(n) % A), optionally with other returns."""
    c = H.make_case(cont, A, n, shared, False)
    if rets is not None:
        c.rets = rets
    return c


def per_sample(c, dtype):
    """(logp, value, x, ratio) of the case in `dtype`; x = logp - old_logp."""
    P = {k: v.to(dtype) for k, v in c.params.items()}
    ha = c.ha.to(dtype)
    hc = ha if c.shared else c.hc.to(dtype)
    _, logp, _, v, _ = H.forward(c, ha, hc, P, dtype)
    x = logp - c.old_logps.to(dtype)
    return logp, v, x, torch.exp(x)


def clipped_count(r, clip):
    return int(((r - 1.0).abs() > clip).sum())


def reference(c):
    """The eight sums in float64, the per-sample references and the bound of every slot (see the module docstring):
    slot 1: sum |expm1(x_i)| tau_i + tau_i^2 / 2 (the derivative of expm1(x) - x is expm1(x)); slot 5: sum sigma_i; slot 6:
    sum 2 |e_i| sigma_i + sigma_i^2; slots 0, 2 exact; 3, 4 double sums of exact terms (1e-12 relative); slot 7 1e-5 relative."""
    logp, v, x, r = per_sample(c, torch.float64)
    ret = c.rets.double()
    e = ret - v
    n = c.n
    tau = ATOL + RTOL * logp.abs()
    sigma = ATOL + RTOL * v.abs()
    # slots 3, 4: the terms are exact in double (fp32 inputs), so the reference is the exactly rounded sum
    sums = [float(n), float((torch.expm1(x) - x).sum()), float(clipped_count(r, c.hyper["ppo_clip"])), math.fsum(ret.tolist()),
            math.fsum((ret * ret).tolist()), float(e.sum()), float((e * e).sum()), float(r.max())]
    bounds = [0.0, float((torch.expm1(x).abs() * tau + tau * tau / 2).sum()), 0.0, 1e-12 * abs(sums[3]),
              1e-12 * sums[4], float(sigma.sum()), float((2 * e.abs() * sigma + sigma * sigma).sum()), RTOL * sums[7]]
    return {"sums": sums, "bounds": bounds, "logp": logp, "value": v, "tau": tau, "sigma": sigma}


def explained_variance_bound(ref):
    """What the slot bounds allow ExplainedVariance = 1 - Var(e) / Var(ret) to move by (first order in each slot, the
    denominator taken at its lower end): Var = s2 / n - (s1 / n)^2, so dVar <= b2 / n + 2 |s1 / n| b1 / n + (b1 / n)^2."""
    s, b = ref["sums"], ref["bounds"]
    n = s[0]
    var_r = s[4] / n - (s[3] / n) ** 2
    var_e = s[6] / n - (s[5] / n) ** 2
    d_r = b[4] / n + 2 * abs(s[3] / n) * b[3] / n + (b[3] / n) ** 2
    d_e = b[6] / n + 2 * abs(s[5] / n) * b[5] / n + (b[5] / n) ** 2
    lo = var_r - d_r
    assert lo > 0
    return d_e / lo + (var_e + d_e) * d_r / (var_r * lo), 1.0 - var_e / var_r


def direct_diag(x, ret, v, clip):
    """The four reported numbers straight from per-sample float64 tensors (no sums of squares)."""
    r = torch.exp(x)
    e = ret - v
    var_r = float(((ret - ret.mean()) ** 2).mean())
    ev = 1.0 - float(((e - e.mean()) ** 2).mean()) / var_r if var_r != 0 else math.nan
    return {"ApproxKL": float((torch.expm1(x) - x).mean()), "ClipFraction": clipped_count(r, clip) / len(x),
            "ExplainedVariance": ev, "RatioMax": float(r.max())}
