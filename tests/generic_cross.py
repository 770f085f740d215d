"""Cell table of tests/test_generic_cross_gpu.py: the nets create_net builds on GenericPPO (nn/generic.py) crossed with both head families,
the value loss, the hyper-parameters, the update options (VALUE_CLIP / ENTROPY_BONUS_SPLIT), the diagnostics and the micro-batching, the
inputs of a cell and its float64 statement (oracle/ddrl_oracle_nav.py with the knobs).  No GPU and no torch.cuda: the table can be inspected
(and its own claims checked, tests/test_generic_cross_cpu.py) anywhere."""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

import heads_ref as H
import loss_options_ref as LR
from ddrl4nav_amd.utils.recipe import hash_weights, sample_uniform
from oracle import ddrl_oracle_nav as N

# ---- factor levels ---------------------------------------------------------------------------------------------------------------------
NETS = ["mlp_split", "mlp_shared", "navpre_shared", "navped_shared", "nav1d_split"]      # what runner/utils.py:_create_generic_net builds
HEADS = [
    "cat5",      # categorical, A <= 6: head weights in registers (the nav fixtures' head)
    "cat9",      # categorical, A > 8: head weights in LDS + head_wgrad_kernel; no net has run it
    "gauss1",    # Gaussian, D = 1: one mean, one log_std
    "gauss3",    # Gaussian, D = 3: an odd D above the fixtures' 2
]
SMOOTH_L1 = [0, 1]
HYPERS = ["default", "other"]          # other: heads_ref.OTHER_HYPER and CLIP_GRID off
OPTIONS = ["none", "clip", "split", "both"]        # VALUE_CLIP, ENTROPY_BONUS_SPLIT
DIAG = [0, 1]                          # PPO_DIAGNOSTICS
BATCHES = [
    (37, 37),      # one chunk, below 128 rows: the f32 dense family
    (131, 131),    # one chunk, the fp16-plane dense family (ops.Linear.uses_planes)
    (150, 131),    # a plane chunk and a 19-row f32 chunk accumulated into one gradient
    (7, 3),        # chunks of 3, 3 and 1
]
FACTORS = [("net", NETS), ("head", HEADS), ("smooth_l1", SMOOTH_L1), ("hyper", HYPERS), ("options", OPTIONS), ("diag", DIAG),
           ("batch", BATCHES)]

Cell = namedtuple("Cell", "net head smooth_l1 hyper options diag n max_batch")

VALUE_CLIP = LR.VALUE_CLIP
CLIP_GRAD_NUM = 0.5          # config_nn.CLIP_GRID_NUM
DUAL_ROWS = (2, 5)           # negative-advantage rows placed in the dual-clip branch (row 2 alone below 37 samples)
DUAL_RATIO = {"default": 3.5, "other": 2.5}


def _cell(net, head, smooth, hyper, options, diag, batch):
    n, cap = BATCHES[batch]
    return Cell(NETS[net], HEADS[head], smooth, HYPERS[hyper], OPTIONS[options], diag, n, cap)


# A pairwise covering array over the seven factors: all 20 (net, head) pairs once, the other five columns placed by search.
# tests/test_generic_cross_cpu.py checks the cover by enumeration.
CELLS = [
    #     net head smooth hyper options diag batch
    _cell(0, 0, 0, 0, 3, 0, 1),
    _cell(0, 1, 1, 0, 1, 0, 2),
    _cell(0, 2, 1, 1, 0, 1, 3),
    _cell(0, 3, 1, 1, 2, 1, 0),
    _cell(1, 0, 1, 0, 3, 1, 3),
    _cell(1, 1, 1, 1, 0, 0, 1),
    _cell(1, 2, 0, 0, 2, 0, 0),
    _cell(1, 3, 0, 0, 1, 1, 2),
    _cell(2, 0, 0, 1, 1, 0, 0),
    _cell(2, 1, 0, 0, 2, 1, 1),
    _cell(2, 2, 1, 0, 3, 0, 2),
    _cell(2, 3, 0, 1, 0, 0, 3),
    _cell(3, 0, 0, 1, 2, 0, 2),
    _cell(3, 1, 1, 0, 1, 0, 3),
    _cell(3, 2, 0, 1, 0, 0, 0),
    _cell(3, 3, 0, 1, 3, 1, 1),
    _cell(4, 0, 0, 0, 0, 0, 2),
    _cell(4, 1, 0, 1, 3, 1, 0),
    _cell(4, 2, 0, 1, 1, 0, 1),
    _cell(4, 3, 1, 0, 2, 1, 3),
]


def levels(cell):
    """The cell's level of every factor of FACTORS, in that order."""
    return (cell.net, cell.head, cell.smooth_l1, cell.hyper, cell.options, cell.diag, (cell.n, cell.max_batch))


def uncovered_pairs(cells=None):
    """[(factor a, level, factor b, level)] that no cell holds: empty for a pairwise covering array."""
    have = [levels(c) for c in (CELLS if cells is None else cells)]
    missing = []
    for a in range(len(FACTORS)):
        for b in range(a + 1, len(FACTORS)):
            seen = {(lv[a], lv[b]) for lv in have}
            missing += [(FACTORS[a][0], x, FACTORS[b][0], y) for x in FACTORS[a][1] for y in FACTORS[b][1] if (x, y) not in seen]
    return missing


def cell_id(cell):
    return "%s-%s-%s-%s-%s-%s-n%d-mb%d" % (cell.net, cell.head, "huber" if cell.smooth_l1 else "mse", cell.hyper, cell.options,
                                           "diag" if cell.diag else "nodiag", cell.n, cell.max_batch)


def cell_seed(cell):
    """One seed per cell, from its own fields (mixed radix: no two cells share one)."""
    s = 0
    for (_, lv), x in zip(FACTORS, levels(cell)):
        s = s * len(lv) + (lv.index(x) if x in lv else len(lv) + zlib.crc32(repr(x).encode()) % 997)    # a level outside the table:
    return 7000 + s                                                                                   # tests/test_generic_learn_loop_gpu.py


# ---- what a cell means -----------------------------------------------------------------------------------------------------------------
def shared(cell):
    return cell.net.endswith("_shared")


def gaussian(cell):
    return cell.head.startswith("gauss")


def n_out(cell):
    return int(cell.head[5:] if gaussian(cell) else cell.head[3:])


def hyper(cell):
    return dict(H.DEFAULT_HYPER if cell.hyper == "default" else H.OTHER_HYPER)


def clip_grad(cell):
    """(CLIP_GRID, CLIP_GRID_NUM)"""
    return (cell.hyper == "default", CLIP_GRAD_NUM)


def options(cell):
    """(value_clip or 0.0, entropy_split)"""
    return (VALUE_CLIP if cell.options in ("clip", "both") else 0.0, cell.options in ("split", "both"))


def chunks(cell):
    """[(lo, hi)] of the micro-batches learn() and forward() cut the batch into."""
    return [(lo, min(cell.n, lo + cell.max_batch)) for lo in range(0, cell.n, cell.max_batch)]


def env_config(cell):
    """(config_env, TASK_TYPE) that make create_net build the cell's net."""
    head = {"discrete_action": False, "act_dim": n_out(cell)} if gaussian(cell) else \
        {"discrete_action": True, "discrete_actions": list(range(n_out(cell)))}
    if cell.net.startswith("mlp"):
        return dict(head, input_dim=4), "classical"
    ped = {"navpre_shared": 0, "navped_shared": 3, "nav1d_split": 3}[cell.net]
    return dict(head, image_batch=1, ped_sim={"total": ped}), "robot_nav"


def config_nn_fields(cell):
    """{config_nn attribute: value} of the cell; TRAINING_ITER_TIME = 1 (one update per cell)."""
    h, (vc, split) = hyper(cell), options(cell)
    out = {"SHARE_CNN_NET": shared(cell), "TRAINING_ITER_TIME": 1, "SMOOTH_L1_LOSS": bool(cell.smooth_l1), "CLIP_GRID": clip_grad(cell)[0],
           "PPO_CLIP": h["ppo_clip"], "DUEL_PPO_CLIP": h["dual_clip"], "V_LOSS_THETA": h["v_loss_theta"],
           "ENTROPY_LOSS_THETA": h["ent_loss_theta"]}
    if vc > 0:
        out["VALUE_CLIP"] = vc
    if split:
        out["ENTROPY_BONUS_SPLIT"] = True
    if cell.diag:
        out["PPO_DIAGNOSTICS"] = True
    return out


def is_buildable(cell):
    """create_net's rules (runner/utils.py) and GenericPPO's for the fields a cell sets."""
    kind, sharing = cell.net.rsplit("_", 1)
    return (cell.net in NETS and cell.head in HEADS and (kind, sharing) in (("mlp", "split"), ("mlp", "shared"), ("navpre", "shared"),
                                                                              ("navped", "shared"), ("nav1d", "split"))
            and 1 <= n_out(cell) <= 18 and 1 <= cell.max_batch <= cell.n and cell.options in OPTIONS and cell.hyper in HYPERS)


def oracle_net(cell, weights=None, dtype=torch.float64):
    """The cell's net in the oracle, recipe weights loaded."""
    pre = {"mlp": lambda: N.MLPPreNet(4, 512), "navpre": lambda: N.NavPreNet(1), "navped": lambda: N.NavPedPreNet(4),
           "nav1d": lambda: N.NavPreNet1D(3)}[cell.net.rsplit("_", 1)[0]]
    net = N.OracleNet(pre, n_out(cell), gaussian(cell), shared(cell))
    if weights is None:
        weights = hash_weights([(k, tuple(p.shape)) for k, p in net.named_parameters()], cell_seed(cell))
    net.load_weights(weights)
    return net.to(dtype)


def encoders(net):
    """The oracle net's encoders in GenericPPO._encs order."""
    return [net.prenet] if net.shared else [net.actor.pre, net.critic.pre]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
class _Stream:
    """Counter-based draws (utils.recipe.sample_uniform): one stream id per call, so that no draw depends on how many came before it
    in ANOTHER tensor."""

    def __init__(self, seed):
        self.seed, self.k = seed, 0

    def uniform(self, *shape):
        self.k += 1
        return sample_uniform(self.seed, self.k, int(np.prod(shape))).astype(np.float64).reshape(shape)

    def normal(self, *shape):
        u1, u2 = self.uniform(*shape), self.uniform(*shape)
        return np.sqrt(-2.0 * np.log1p(-u1)) * np.cos(2.0 * np.pi * u2)


def _states(cell, s):
    """float32 states with the ranges of the nav fixtures (tests/golden/make_golden_nav.py), shaped as the encoders' docstrings say."""
    n, f = cell.n, np.float32
    kind = cell.net.rsplit("_", 1)[0]
    if kind == "mlp":
        return [s.normal(n, 4).astype(f)]
    if kind == "nav1d":
        laser = (0.05 + 0.95 * s.uniform(n, 1, 960)).astype(f)
        vec = s.normal(n, 5).astype(f)
        ped = ((s.uniform(n, 3, 48, 48) < 0.15) * (0.5 + 0.5 * s.uniform(n, 3, 48, 48))).astype(f)
        return [laser, vec, ped]
    img = (s.uniform(n, 1, 48, 48) < 0.3).astype(f)
    vec = s.normal(n, 9).astype(f)
    if kind == "navped":
        return [img, vec, (s.uniform(n, 3, 48, 48) < 0.1).astype(f)]
    return [img, vec]


def _threads():
    import parity_util as P
    return P.oracle_threads()


def forward64(cell, weights, states, actions):
    """(dist_out, logp, entropy per element, value [n]) of the float64 oracle, float64 numpy; the categorical clamp is float32's eps
    (oracle_nav.losses)."""
    from oracle.ddrl_oracle import EPS, categorical_entropy, categorical_log_prob
    net = oracle_net(cell, weights)
    threads = torch.get_num_threads()
    torch.set_num_threads(_threads())
    try:
        with torch.no_grad():
            st = [torch.from_numpy(x).double() for x in states]
            a = torch.from_numpy(np.asarray(actions)).double()
            dist, logp, ent, v = net(st, a)
            if not net.gaussian:
                p_hat = dist / dist.sum(-1, keepdim=True)
                logits = torch.log(torch.clamp(p_hat, EPS, 1.0 - EPS))
                logp, ent = categorical_log_prob(logits, a), categorical_entropy(p_hat, logits)
    finally:
        torch.set_num_threads(threads)
    return dist.numpy(), logp.numpy(), ent.numpy(), v.numpy()[:, 0]


Inputs = namedtuple("Inputs", "weights states actions old_logps advs rets old_values logp64 v64 dist64 ent64")

MARGIN = 2e-3          # what the redraws keep clear of a branch boundary; the promises (check_recipe) ask for 1e-3
# cell id -> another seed offset for the cell's inputs, where the first ones break a promise of tests/test_generic_cross_cpu.py
SALT = {
    # the fp32 oracle's own prenet.conv1.bias gradient (a sum over 150 x 48 x 48 signed terms per channel) came out 1.2e-5 max|g64| from
    # float64 on the first inputs, past half the GPU bound; 6.6e-6 on these
    "navped_shared-cat5-mse-other-split-nodiag-n150-mb131": 2,
}


def _ratio_margin(ratio, h):
    b = np.array([1.0 - h["ppo_clip"], 1.0 + h["ppo_clip"], h["dual_clip"]])
    return np.abs(ratio[:, None] - b[None, :]).min(1)


@functools.lru_cache(maxsize=None)
def cell_inputs(cell):
    """Inputs of a cell, following tests/golden/make_golden_nav.py:run_case: actions drawn from the float64 oracle's own distribution,
    old_logps = its log-prob + N(0, 0.3), advantages N(0, 1) with one exact zero, rets = v64 + advs; DUAL_ROWS placed at ratio
    DUAL_RATIO under a negative advantage; old_values = v64 - d, d / VALUE_CLIP cycling through loss_options_ref.D_OVER_C.  A row whose
    ratio (or, for the Huber loss, |ret - v|) lands within MARGIN of a branch boundary draws its noise again, from the float64 numbers
    alone."""
    seed = cell_seed(cell) + 100003 * SALT.get(cell_id(cell), 0)
    s = _Stream(seed)
    n, h = cell.n, hyper(cell)
    probe = oracle_net(cell, dtype=torch.float32)
    weights = hash_weights([(k, tuple(p.shape)) for k, p in probe.named_parameters()], cell_seed(cell))
    states = _states(cell, s)
    D = n_out(cell)
    if gaussian(cell):
        mu, _, _, _ = forward64(cell, weights, states, np.zeros((n, D)))
        std = np.exp(weights["actor.log_std"].astype(np.float64))
        actions = (mu + std * s.normal(n, D)).astype(np.float32)
    else:
        probs, _, _, _ = forward64(cell, weights, states, np.zeros(n))
        cdf = np.cumsum(probs / probs.sum(1, keepdims=True), axis=1)
        actions = np.minimum((s.uniform(n)[:, None] >= cdf).sum(1), D - 1).astype(np.float32)
    dist64, logp64, ent64, v64 = forward64(cell, weights, states, actions)
    old = (logp64 + 0.3 * s.normal(n)).astype(np.float32)
    advs = s.normal(n).astype(np.float32)
    dual = [r for r in DUAL_ROWS if r < n and (n >= 37 or r == DUAL_ROWS[0])]
    for r in dual:
        advs[r] = -(1.5 + abs(advs[r]))
        old[r] = np.float32(logp64[r] - np.log(DUAL_RATIO[cell.hyper]))
    advs[1] = 0.0
    for _ in range(16):      # redraw the rows that sit on a boundary
        bad = _ratio_margin(np.exp(logp64 - old.astype(np.float64)), h) < MARGIN
        bad[dual] = False
        if not bad.any():
            break
        old[bad] = (logp64 + 0.3 * s.normal(n)).astype(np.float32)[bad]
    for _ in range(16):
        bad = np.abs(np.abs(advs.astype(np.float64)) - 1.0) < MARGIN       # never a placed row: those are at 0 or beyond 1.5
        if not bad.any():
            break
        advs[bad] = s.normal(n).astype(np.float32)[bad]
    rets = (v64 + advs).astype(np.float32)
    d_over_c = np.array([LR.D_OVER_C[LR.d_index(i)] for i in range(n)])
    old_values = (v64 - d_over_c * VALUE_CLIP).astype(np.float32)
    return Inputs(weights, states, actions, old, advs, rets, old_values, logp64, v64, dist64, ent64)


def check_recipe(cell, x):
    """The recipe's promises, in float64 (tests/test_generic_cross_cpu.py runs them for every cell)."""
    h, n = hyper(cell), cell.n
    adv = x.advs.astype(np.float64)
    assert (adv > 0).any() and (adv < 0).any() and (adv == 0).sum() >= 1
    ratio = np.exp(x.logp64 - x.old_logps.astype(np.float64))
    lo, hi, dual = 1.0 - h["ppo_clip"], 1.0 + h["ppo_clip"], h["dual_clip"]
    assert float(_ratio_margin(ratio, h).min()) > 1e-3, float(_ratio_margin(ratio, h).min())
    assert ((ratio > dual) & (adv < 0)).any(), "no row in the dual-clip branch"
    if n >= 37:
        assert (ratio < lo).any() and ((ratio > lo) & (ratio < hi)).any() and ((ratio > hi) & (ratio < dual)).any()
    err = x.rets.astype(np.float64) - x.v64
    if cell.smooth_l1:
        assert (np.abs(err) < 1.0).any() and (np.abs(err) > 1.0).any()
        assert float(np.abs(np.abs(err) - 1.0).min()) > 1e-3, float(np.abs(np.abs(err) - 1.0).min())
    if options(cell)[0] > 0:
        c = options(cell)[0]
        el = lambda e: LR.element(torch.from_numpy(e), bool(cell.smooth_l1)).numpy()
        d = x.v64 - x.old_values.astype(np.float64)
        v_c = x.old_values.astype(np.float64) + np.clip(d, -c, c)
        l_u, l_c = el(err), el(x.rets.astype(np.float64) - v_c)
        assert float(np.abs(np.abs(d) - c).min()) > 1e-3
        clipped = np.abs(d) > c
        assert clipped.any() and (~clipped).any()
        assert float(np.abs(l_u - l_c)[clipped].min()) > 1e-4, float(np.abs(l_u - l_c)[clipped].min())
        if cell.smooth_l1:
            assert float(np.abs(np.abs(x.rets.astype(np.float64) - v_c) - 1.0).min()) > 1e-3
        if n >= 33:     # both sides of the maximum among the clipped samples
            assert (l_u > l_c)[clipped].any() and (l_u < l_c)[clipped].any()


# ---- the float64 statement of one update ---------------------------------------------------------------------------------------------------
Update = namedtuple("Update", "net losses grads norm coef")


def oracle_update(cell, x, dtype=torch.float64, sub=None, record=None):
    """One loss + backward of the oracle on the cell, in `dtype`, under the cell's knobs.  sub / record: per encoder (encoders() order)
    the dicts of oracle_nav._act.  -> Update(net with .grad, [total, actor, v, entropy], {name: gradient or None}, float64 norm of the
    whole gradient, clip coefficient)."""
    net = oracle_net(cell, x.weights, dtype)
    for i, e in enumerate(encoders(net)):
        if sub is not None:
            e.sub = sub[i]
        if record is not None:
            e.record = record[i]
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    vc, split = options(cell)
    threads = torch.get_num_threads()
    torch.set_num_threads(_threads())
    try:
        parts = N.losses(net, [t(s) for s in x.states], t(x.actions), t(x.old_logps), t(x.advs), t(x.rets), hyper=hyper(cell),
                         smooth_l1=bool(cell.smooth_l1), value_clip=vc, old_values=t(x.old_values) if vc > 0 else None)
        N.backward(net, *parts, hyper=hyper(cell), entropy_split=split)
    finally:
        torch.set_num_threads(threads)
    grads = {k: (None if p.grad is None else p.grad.detach().double().numpy()) for k, p in net.named_parameters()}
    flat = torch.cat([torch.from_numpy(g).reshape(-1) for g in grads.values() if g is not None])
    on, max_norm = clip_grad(cell)
    norm, coef = H.clip_coef64(flat, max_norm, on)
    return Update(net, [p.item() for p in parts], grads, norm, coef)


def relu_of(record):
    """{site: relu(z)} of a recorded forward: the `sub` that makes another oracle run take these decisions."""
    return {k: torch.relu(z) for k, z in record.items()}
