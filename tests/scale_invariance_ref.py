"""Power-of-two re-scalings of a net's layers under which every output is known bit for bit (test infrastructure, numpy only).

The nets are positively homogeneous layer by layer (leaky-ReLU, ReLU, max-pool) and every scale of the fp16 plane scheme is a power
of two (csrc/common.h f16_scale, WGRAD_HEADROOM, the per-sample g_s and g_max), so multiplying the weight of layer l of encoder e by
2^k[e][l] -- its bias by the cumulative 2^(k[e][1] + ... + k[e][l]), and the head weights by 2^-K[e], K[e] the encoder's sum --
leaves logits, value, probabilities and losses unchanged and multiplies every intermediate tensor and every gradient by an exactly
known power of two: in fp32 and in the planes alike, as long as nothing overflows, goes subnormal or meets a clamp.  The clamps, by
name: PLANE_SCALE_EXP_MAX (csrc/common.h: no plane scale above 2^40, met by a maximum below 2^-27), GSC_EXP_MIN / GSC_EXP_MAX (+-60:
the per-sample gradient scale g_s), the 0x1p60f caps of the operator path's scale_of_amax (csrc/engine2.h, csrc/fconv.hip).  The
preconditions below keep every transformed tensor far from all of them.

A kernel that un-scales with another slot or another encoder's slot than the one its operand was packed with breaks the equality
at once; weights that all sit in one binade (the init recipe) cannot show that.

atari_transform(weights, exps)   -> (transformed weights, table)         the Atari arena (recipe.make_weights dict)
nav_transform(name, weights)     -> (transformed weights, table)         the operator-composed nets (nn/generic.py), NAV_PLANS
table: {"param": {name: exponent}, "grad": {name: exponent}, "debug": {(buffer, encoder): exponent},
        "amax": {slot: [exponent per encoder]}}   (debug / amax: the Atari context's HotPath.debug_buffer / plane_maxima)
"""
import numpy as np

ATARI_LAYERS = ("conv1", "conv2", "conv3", "linear")

# exponents k[e][l], l = conv1, conv2, conv3, linear
SETS = {
    "A": {"actor": (+3, -2, +5, -4), "critic": (-3, +4, -6, +1)},      # the base two-encoder case
    "B": {"actor": (-3, +4, -6, +1), "critic": (+3, -2, +5, -4)},      # A with the encoders swapped: both directions of every mix-up
    "S": {"shared": (+4, -5, +3, +2)},                                 # one shared prenet
}
MAX_CUMULATIVE = 12          # |cumulative exponent| of every layer
MIN_ENCODER_GAP = 5          # binades between the two encoders of every weight slot (sets A and B)
MIN_WEIGHT_MAX_LOG2 = -20    # every transformed weight maximum >= 2^-20: seven binades above PLANE_SCALE_EXP_MAX's 2^-27

_F32_TINY = float(np.finfo(np.float32).tiny)


def scale_pow2(a, k):
    """a x 2^k in the dtype of a, asserted exact: finite, and no non-zero element below the normal range."""
    a = np.asarray(a)
    out = np.ldexp(a, int(k)).astype(a.dtype)
    assert np.isfinite(out).all(), "2^%d overflows" % k
    nz = a != 0
    tiny = _F32_TINY if a.dtype == np.float32 else float(np.finfo(a.dtype).tiny)
    assert not nz.any() or float(np.abs(out[nz]).min()) >= tiny, "2^%d leaves the normal range" % k
    return out


def bits(a):
    """The bit pattern of a float array as integers (what the equality asserts compare)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _encoders(weights):
    """[(encoder key in an exponent set, parameter prefix, encoder index of the context)]"""
    if any(k.startswith("prenet.") for k in weights):
        return [("shared", "prenet.", 0)]
    return [("actor", "actor.pre.", 0), ("critic", "critic.pre.", 1)]


def check_atari_preconditions(weights, exps, transformed):
    encs = _encoders(weights)
    assert sorted(exps) == sorted(e for e, _, _ in encs), (sorted(exps), encs)
    for e, pre, _ in encs:
        k = exps[e]
        assert len(k) == len(ATARI_LAYERS)
        assert all(abs(c) <= MAX_CUMULATIVE for c in np.cumsum(k)), (e, np.cumsum(k))
        for layer in ATARI_LAYERS:
            m = float(np.abs(transformed[pre + layer + ".weight"]).max())
            assert m >= 2.0 ** MIN_WEIGHT_MAX_LOG2, (pre + layer, m)
    if len(encs) == 2:
        for l in range(len(ATARI_LAYERS)):
            assert abs(exps["actor"][l] - exps["critic"][l]) >= MIN_ENCODER_GAP, (ATARI_LAYERS[l], exps)
    for name in ("actor.actor_linear.weight", "critic.critic_linear.weight"):
        assert float(np.abs(transformed[name]).max()) >= 2.0 ** MIN_WEIGHT_MAX_LOG2, name


def atari_transform(weights, exps):
    """weights: recipe.make_weights dict (two encoders or one shared); exps: one entry of SETS.  -> (transformed weights, table)."""
    encs = _encoders(weights)
    param = {k: 0 for k in weights}
    grad = {k: 0 for k in weights}
    debug, amax = {}, {s: [0, 0] for s in ("wl", "w2", "w3", "w1", "a1", "a2", "a3", "dh", "dz3", "dz2", "dz1", "gmax")}
    K = {}
    for e, pre, idx in encs:
        k = [int(x) for x in exps[e]]
        c = [int(x) for x in np.cumsum(k)]
        K[e] = c[-1]
        for l, layer in enumerate(ATARI_LAYERS):
            param[pre + layer + ".weight"], param[pre + layer + ".bias"] = k[l], c[l]
            grad[pre + layer + ".weight"], grad[pre + layer + ".bias"] = -k[l], -c[l]
        # HotPath.debug_buffer: 0 a1, 1 a2, 2 a3, 3 h scale by the cumulative exponent; 4 dz1, 5 dz2, 6 dz3, 7 dh (returned as the
        # TRUE gradients) by its negative
        for l in range(4):
            debug[(l, idx)] = c[l]
            debug[(4 + l, idx)] = -c[l]
        # 13: the per-sample scale g_s = 2^floor(log2 max|dh_s|) follows dh
        debug[(13, idx)] = -c[3]
        # plane_maxima: weight slots by their layer's exponent; a1's bound (sum |w1| + |b1|) and the measured a2 / a3 maxima by the
        # cumulative one; the gradient slots hold the maxima of the tensors NORMALISED by g_s, which follows dh: dh's own slot
        # is unchanged, dz_l's scales by what lies between it and dh; gmax = the largest g_s
        for slot, x in (("w1", k[0]), ("w2", k[1]), ("w3", k[2]), ("wl", k[3]), ("a1", c[0]), ("a2", c[1]), ("a3", c[2]),
                        ("dh", 0), ("dz3", c[3] - c[2]), ("dz2", c[3] - c[1]), ("dz1", c[3] - c[0]), ("gmax", -c[3])):
            amax[slot][idx] = x
    ka = K["shared"] if "shared" in K else K["actor"]
    kc = K["shared"] if "shared" in K else K["critic"]
    param["actor.actor_linear.weight"], grad["actor.actor_linear.weight"] = -ka, ka
    param["critic.critic_linear.weight"], grad["critic.critic_linear.weight"] = -kc, kc
    debug[(8, 0)] = debug[(9, 0)] = 0          # dlogits, dvalue
    out = {name: scale_pow2(w, param[name]) for name, w in weights.items()}
    check_atari_preconditions(weights, exps, out)
    return out, {"param": param, "grad": grad, "debug": debug, "amax": amax}


# ---- operator-composed nets (nn/generic.py) -----------------------------------------------------------------------------------------
# Per encoder: `branches` are the layer chains that end in a concatenation (generic.py _NavBase: fc0 and, for NavPreNet1D, fc_1d write
# their slices of the `cat` buffer, the raw vector state joins them there), `post` the layers after it.  The per-sample magnitude
# behind fc1's plane scale is taken over the whole concatenated row, raw vector included, so every branch must arrive with cumulative
# exponent 0 (its last layer cancels the earlier ones); the layers after the concatenation are free and their sum is undone in the
# head weights.  MLPPreNet has no concatenation: its one layer is `post`.  log_std is untouched.
def _plan(branches, post):
    return {"branches": branches, "post": post}


_LASER = ("conv1d1", "conv1d2", "fc_1d.0")
_IMAGE = ("conv1", "conv2", "conv3", "fc0.0")
_POST = ("fc1.0", "fc2")
NAV_PLANS = {
    "f13_nav1d_gauss": {
        "actor.pre.": _plan([list(zip(_LASER, (+3, -5, +2))), list(zip(_IMAGE, (+4, -2, +3, -5)))], list(zip(_POST, (+3, -4)))),
        "critic.pre.": _plan([list(zip(_LASER, (-4, +6, -2))), list(zip(_IMAGE, (-3, +5, -6, +4)))], list(zip(_POST, (-2, +5))))},
    "f14_navped_shared": {
        "prenet.": _plan([list(zip(_IMAGE, (-5, +3, -4, +6)))], list(zip(_POST, (+2, -6))))},
    "f15_mlp_classical": {
        "actor.pre.": _plan([], [("fc0.0", +5)]),
        "critic.pre.": _plan([], [("fc0.0", -4)])},
}


def check_nav_plan(plan):
    for chain in plan["branches"] + [plan["post"]]:
        ks = [k for _, k in chain]
        assert all(2 <= abs(k) <= 6 for k in ks), chain
        assert all(a != b for a, b in zip(ks, ks[1:])), chain
        assert all(abs(c) <= MAX_CUMULATIVE for c in np.cumsum(ks)), chain
    for chain in plan["branches"]:
        assert sum(k for _, k in chain) == 0, ("a branch must reach the concatenation with cumulative exponent 0", chain)


def nav_transform(name, weights):
    """weights: {parameter name: array} of the net of fixture `name` (recipe.hash_weights).  -> (transformed weights, table)."""
    plans = NAV_PLANS[name]
    param = {k: 0 for k in weights}
    grad = {k: 0 for k in weights}
    K = {}
    for pre, plan in plans.items():
        check_nav_plan(plan)
        for chain in plan["branches"] + [plan["post"]]:
            c = 0
            for layer, k in chain:
                c += k
                param[pre + layer + ".weight"], param[pre + layer + ".bias"] = k, c
                grad[pre + layer + ".weight"], grad[pre + layer + ".bias"] = -k, -c
        K[pre] = sum(k for _, k in plan["post"])
    ka = K["prenet."] if "prenet." in K else K["actor.pre."]
    kc = K["prenet."] if "prenet." in K else K["critic.pre."]
    param["actor.actor_linear.weight"], grad["actor.actor_linear.weight"] = -ka, ka
    param["critic.critic_linear.weight"], grad["critic.critic_linear.weight"] = -kc, kc
    touched = {k for k, v in param.items() if v} | {k[:-len("weight")] + "bias" for k, v in param.items() if v and k.endswith("weight")}
    layers = {k for k in weights if k.endswith(".weight") and "linear" not in k.split(".")[-2]}
    assert layers <= touched, ("every encoder layer takes an exponent", sorted(layers - touched))
    out = {k: scale_pow2(w, param[k]) for k, w in weights.items()}
    for k, w in out.items():
        if k.endswith(".weight"):
            assert float(np.abs(w).max()) >= 2.0 ** MIN_WEIGHT_MAX_LOG2, k
    return out, {"param": param, "grad": grad}


# ---- a seeded PPO batch for the Atari context ----------------------------------------------------------------------------------------
def atari_batch(n, seed=0):
    """(frames u8 [n, 4, 84, 84], actions, old_logps, advs, rets): Pong-like frames in the even rows and uniform random bytes in the
    odd ones; advantages of both signs over four decades; old log-probs near the initial policy's (-log 6), so that most ratios lie
    inside the clip range and a few outside."""
    from ddrl4nav_amd.utils.recipe import pong_frames
    rng = np.random.default_rng(7000 + 31 * n + seed)
    frames = rng.integers(0, 256, size=(n, 4, 84, 84), dtype=np.uint8)
    frames[0::2] = pong_frames(500 + n + seed, (n + 1) // 2)
    actions = rng.integers(0, 6, size=n).astype(np.float32)
    old_logps = (np.full(n, -1.79) + rng.normal(0, 0.1, n)).astype(np.float32)
    advs = (rng.choice(np.array([-1.0, 1.0]), n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
    rets = rng.normal(size=n).astype(np.float32)
    return frames, actions, old_logps, advs, rets


# ---- base weights with a maximum at either end of a binade (f16_scale: frexpf puts a maximum into [2^12, 2^13)) ---------------------
def binade_edge_weights(weights, below):
    """A copy of `weights` in which each encoder weight tensor has ONE element set to the next power of two at or above its largest
    magnitude (below=False: the maximum is the lower end of its binade, frexpf's fraction 0.5) or to nextafter of that value towards
    zero (below=True: the upper end of the binade below, fraction 1 - 2^-24).  The element is the one with the largest magnitude,
    and keeps its sign -- the tensor changes by less than a factor two in one element.  These are other networks than the base."""
    out = {k: v.copy() for k, v in weights.items()}
    planted = {}
    for name, w in out.items():
        if not name.endswith(".weight") or ".pre." not in name and not name.startswith("prenet."):
            continue
        flat = w.reshape(-1)
        i = int(np.abs(flat).argmax())
        m = np.float32(abs(flat[i]))
        fr, ex = np.frexp(m)
        p2 = np.float32(m if fr == 0.5 else np.ldexp(np.float32(1.0), int(ex)))
        v = np.nextafter(p2, np.float32(0.0)) if below else p2
        flat[i] = np.copysign(v, flat[i])
        assert float(np.abs(flat).max()) == float(v)
        planted[name] = (i, float(flat[i]))
    return out, planted
