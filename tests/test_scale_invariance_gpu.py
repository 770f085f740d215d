"""The plane kernels under per-layer, per-encoder power-of-two weight scales (tables: tests/scale_invariance_ref.py, proved on the fp32
oracles in tests/test_scale_invariance_cpu.py).  Every other Atari test loads recipe.make_weights(0), in which both encoders of
every weight slot sit in one binade: a kernel that reads amax_idx(slot, 0) where it means `e`, takes W2's slot for W3's, or packs
with another scale than its consumer un-scales with passes them all.  Here layer l of encoder e is multiplied by 2^k[e][l] and the
heads by 2^-K[e]; the nets are positively homogeneous and every scale of the plane scheme is a power of two, so every output of
the kernels is owed BIT FOR BIT (the ranges: scale_invariance_ref.py).

  a  two ppo_iter on the same weights: bit-equal gradients (the premise)
  b  training iteration (n = 37, 6; two encoders: sets A, B; shared prenet: set S): parameter gradients, losses, a1 a2 a3 h, the
     true dz1 dz2 dz3 dh, g_s, dvalue, dlogits and every plane_maxima() slot bit-equal after the table's power of two
  c  fused acting forward (n = 5, 130)          d  batch-tiled acting forward (n = 513 > ACT_FUSED_MAX)
  e  ddrl_encoder_forward / _backward with a crafted dh whose rows span 2^30
  f  the operator-composed nets f13 / f14 / f15 (branch rule of NAV_PLANS)
Bit-equality ties the scaled runs to the base run; the base run is tied to float64 by the rest of the suite, and here:
  set A against the float64 oracle directly, and base weights whose maxima sit at either end of a binade (f16_scale's frexpf),
  under the per-tensor criterion of F3 / F21: |d| <= 2e-5 max|g64|, cosine > 1 - 1e-9.
Recorded, never asserted (tests/golden/margins.json "scale_invariance/..."): the kernels' error over the fp32 oracle's, per tensor."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import parity_util as P
import scale_invariance_ref as R
from ddrl4nav_amd.utils.recipe import flatten, make_weights
from oracle import ddrl_oracle as O
from test_gpu_parity import _views, dev

pytestmark = pytest.mark.gpu

A1, A2, A3, H = (32, 20, 20), (64, 9, 9), (3136,), (512,)
# HotPath.debug_buffer: activations, h, the data-gradient chain (returned as true gradients) and the per-sample scale g_s
BUFFERS = ((0, A1), (1, A2), (2, A3), (3, H), (4, A1), (5, A2), (6, A3), (7, H), (13, ()))


def _ordered(a):
    """float32 bit patterns as integers that grow with the value: differences are distances in units of the last place."""
    i = R.bits(np.ascontiguousarray(a, np.float32)).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _mismatches(base, other, exps):
    """[report line] for every tensor of `other` that is not `base` x 2^exponent bit for bit."""
    assert sorted(base) == sorted(other) == sorted(exps), (sorted(set(base) ^ set(exps)), sorted(set(base) ^ set(other)))
    bad = []
    for key in sorted(base):
        want = np.ldexp(np.asarray(base[key], np.float32), int(exps[key])).astype(np.float32)
        got = np.asarray(other[key], np.float32)
        assert np.isfinite(base[key]).all(), key
        differ = R.bits(got) != R.bits(want)
        if differ.any():
            fin = np.isfinite(got)
            ulp = int(np.abs(_ordered(got[fin & differ]) - _ordered(want[fin & differ])).max()) if (fin & differ).any() else 0
            line = "%s (x 2^%d): %d of %d elements differ, largest distance %d ulp, non-finite: %s" % (
                key, exps[key], int(differ.sum()), differ.size, ulp, bool((~fin).any()))
            print(line)
            print("  got ", got[differ].ravel()[:8], "\n  want", want[differ].ravel()[:8])
            bad.append(line)
    return bad


def _context(max_batch, shared=False):
    from ddrl4nav_amd.engine import HotPath
    return HotPath(max_batch=max_batch, share_cnn_net=1 if shared else 0).keep_activations()


def _train_snapshot(h, weights, batch, shared):
    """One ppo_iter -> {key: array} of everything section b compares; keys as _train_exponents gives them."""
    frames, actions, old_logps, advs, rets = batch
    n = frames.shape[0]
    h.set_params(flatten(weights, shared=shared))
    h.ppo_iter(dev(frames), dev(actions), dev(old_logps), dev(advs), dev(rets))
    flat = h.grads.cpu().numpy()
    out = {"grad/" + k: v.copy() for k, v in _views(flat[:h.n_params], shared).items()}
    out["losses"] = flat[h.n_params:h.n_params + 3].copy()
    for e in range(1 if shared else 2):
        for which, shape in BUFFERS:
            out["buffer%d/enc%d" % (which, e)] = h.debug_buffer(which, shape, n, e).cpu().numpy()
    out["dlogits"] = h.debug_buffer(8, (6,), n, 0).cpu().numpy()
    out["dvalue"] = h.debug_buffer(9, (), n, 0).cpu().numpy()
    for slot, v in h.plane_maxima().items():
        for e in range(1 if shared else 2):         # a shared prenet leaves encoder 1's slots unwritten
            out["amax/%s/enc%d" % (slot, e)] = v[e:e + 1]
    return out


def _train_exponents(table, shared):
    ex = {"grad/" + k: v for k, v in table["grad"].items()}
    ex.update({"losses": 0, "dlogits": table["debug"][(8, 0)], "dvalue": table["debug"][(9, 0)]})
    for e in range(1 if shared else 2):
        for which, _ in BUFFERS:
            ex["buffer%d/enc%d" % (which, e)] = table["debug"][(which, e)]
        for slot, v in table["amax"].items():
            ex["amax/%s/enc%d" % (slot, e)] = v[e]
    return ex


def _settle_zero_rows(base, got, shared):
    """A sample whose dh row is all zero (its ratio is clipped and nothing else feeds that encoder) has no magnitude to follow: g_s
    keeps 2^GSC_EXP_MIN (csrc/encoder.hip dh_normalise_kernel), a clamp that is really met, in both runs, and multiplies zeros.
    Asserted here; those entries then leave the bit comparison of g_s.  Every other row follows the table."""
    base, got = dict(base), dict(got)
    for e in range(1 if shared else 2):
        zero = ~base["buffer7/enc%d" % e].any(axis=1)
        assert np.array_equal(zero, ~got["buffer7/enc%d" % e].any(axis=1)), e
        key = "buffer13/enc%d" % e
        for d in (base, got):
            assert (d[key][zero] == np.float32(2.0 ** -60)).all(), (e, d[key][zero])
            d[key] = np.where(zero, np.float32(0.0), d[key])
        assert not zero.all(), e
    return base, got


@pytest.fixture(scope="module")
def hp():
    h = _context(64)
    yield h
    h.close()


@pytest.fixture(scope="module")
def hp_shared():
    h = _context(64, shared=True)
    yield h
    h.close()


_BASE = {}


def _base_run(h, n, shared):
    """The base-weight snapshot at n, computed once and left unchanged."""
    key = (n, shared)
    if key not in _BASE:
        _BASE[key] = _train_snapshot(h, make_weights(0, shared=shared), R.atari_batch(n), shared)
    return _BASE[key]


# ---- a ------------------------------------------------------------------------------------------------------------------------
def test_two_iterations_on_the_base_weights_are_bit_equal(hp):
    frames, actions, old_logps, advs, rets = R.atari_batch(37)
    args = (dev(frames), dev(actions), dev(old_logps), dev(advs), dev(rets))
    hp.set_params(flatten(make_weights(0)))
    hp.ppo_iter(*args)
    first = hp.grads.clone()
    hp.ppo_iter(*args)
    assert bool(torch.isfinite(first).all()) and float(first[:hp.n_params].abs().max()) > 0
    assert torch.equal(first, hp.grads)


# ---- b ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,n", [("A", 37), ("B", 37), ("A", 6), ("B", 6)])
def test_training_iteration_two_encoders(hp, which, n):
    """n = 37: ragged against the sample pairs of the weight gradients and the five-sample tiles of the data gradients; n = 6: a
    weight-gradient split holds fewer samples than splits exist."""
    base = _base_run(hp, n, False)
    wt, table = R.atari_transform(make_weights(0), R.SETS[which])
    got = _train_snapshot(hp, wt, R.atari_batch(n), False)
    for k, v in base.items():
        if k.startswith("grad/") or k.startswith("buffer"):
            assert np.abs(v).max() > 0, k
    base, got = _settle_zero_rows(base, got, False)
    bad = _mismatches(base, got, _train_exponents(table, False))
    assert not bad, "\n".join(bad)


def test_training_iteration_shared_prenet(hp_shared):
    n = 37
    base = _base_run(hp_shared, n, True)
    wt, table = R.atari_transform(make_weights(0, shared=True), R.SETS["S"])
    got = _train_snapshot(hp_shared, wt, R.atari_batch(n), True)
    base, got = _settle_zero_rows(base, got, True)
    bad = _mismatches(base, got, _train_exponents(table, True))
    assert not bad, "\n".join(bad)


# ---- c, d ---------------------------------------------------------------------------------------------------------------------
def _acting_snapshot(h, weights, frames, keep):
    n = frames.shape[0]
    h.set_params(flatten(weights))
    probs, value, action, logp = h.forward(dev(frames), act=None, seed=77, stream_id=3)
    out = {"probs": probs.cpu().numpy(), "value": value.cpu().numpy(), "action": action.cpu().numpy(), "logp": logp.cpu().numpy()}
    for e in (0, 1):
        for which, shape in BUFFERS[:4] if keep else BUFFERS[2:4]:      # a1 / a2 stay on chip unless the context keeps them
            out["buffer%d/enc%d" % (which, e)] = h.debug_buffer(which, shape, n, e).cpu().numpy()
    return out


def _acting_exponents(table, keys):
    ex = {k: 0 for k in ("probs", "value", "action", "logp")}
    for k in keys:
        if k.startswith("buffer"):
            which, e = int(k[6:k.index("/")]), int(k[-1])
            ex[k] = table["debug"][(which, e)]
    return ex


@pytest.fixture(scope="module")
def hp_act():
    h = _context(130)
    yield h
    h.close()


@pytest.mark.parametrize("n", [5, 130])
def test_fused_acting_forward(hp_act, n):
    frames = R.atari_batch(n, seed=1)[0]
    base = _acting_snapshot(hp_act, make_weights(0), frames, True)
    assert len(np.unique(base["action"])) > 1 and np.abs(base["buffer0/enc1"]).max() > 0
    for which in ("A", "B"):
        wt, table = R.atari_transform(make_weights(0), R.SETS[which])
        got = _acting_snapshot(hp_act, wt, frames, True)
        bad = _mismatches(base, got, _acting_exponents(table, base))
        assert not bad, which + "\n" + "\n".join(bad)


def test_batch_tiled_acting_forward():
    """n = 513 on a context of that capacity: above ACT_FUSED_MAX, the batch-tiled kernels and the split dense layer."""
    from ddrl4nav_amd.engine import HotPath
    n = 513
    frames = R.atari_batch(n, seed=2)[0]
    h = HotPath(max_batch=n)
    try:
        base = _acting_snapshot(h, make_weights(0), frames, False)
        for which in ("A", "B"):
            wt, table = R.atari_transform(make_weights(0), R.SETS[which])
            got = _acting_snapshot(h, wt, frames, False)
            bad = _mismatches(base, got, _acting_exponents(table, base))
            assert not bad, which + "\n" + "\n".join(bad)
    finally:
        h.close()


# ---- e ------------------------------------------------------------------------------------------------------------------------
def test_encoder_only_entry_points():
    """ddrl_encoder_forward / ddrl_encoder_backward on a shared context with a crafted dh whose row maxima span 2^30; the injected
    dh is scaled by its predicted exponent (-K)."""
    from ddrl4nav_amd._lib import check
    from ddrl4nav_amd.engine import HotPath, _stream
    n = 8
    frames = dev(R.atari_batch(n, seed=3)[0])
    rng = np.random.default_rng(88)
    dh = (rng.normal(size=(n, 512)) * 2.0 ** np.linspace(-24, 6, n)[:, None]).astype(np.float32)
    dh[:, ::7] = 0.0
    w = make_weights(0, shared=True)
    wt, table = R.atari_transform(w, R.SETS["S"])
    h = HotPath(max_batch=n, share_cnn_net=1)
    try:
        def run(weights, dh_in):
            h.set_params(flatten(weights, shared=True))
            h.grads.zero_()
            check(h.lib.ddrl_encoder_forward(h.ctx, c_void_p(frames.data_ptr()), n, _stream()))
            h.debug_view(7, H, n, 0).copy_(torch.from_numpy(dh_in))
            check(h.lib.ddrl_encoder_backward(h.ctx, c_void_p(frames.data_ptr()), n, _stream()))
            torch.cuda.synchronize()
            out = {"grad/" + k: v.copy() for k, v in _views(h.grads[:h.n_params].cpu().numpy(), True).items() if k.startswith("prenet.")}
            for which, shape in BUFFERS[:3] + BUFFERS[4:]:
                out["buffer%d/enc0" % which] = h.debug_buffer(which, shape, n, 0).cpu().numpy()
            return out

        base = run(w, dh)
        got = run(wt, R.scale_pow2(dh, table["debug"][(7, 0)]))
        assert all(np.abs(v).max() > 0 for v in base.values())
        ex = {k: (table["grad"][k[5:]] if k.startswith("grad/") else table["debug"][(int(k[6:k.index("/")]), 0)]) for k in base}
        bad = _mismatches(base, got, ex)
        assert not bad, "\n".join(bad)
    finally:
        h.close()


# ---- f ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.NAV_PLANS))
def test_operator_composed_nets(golden, name):
    from test_generic_gpu import _make, _states
    g = golden(name)
    net, w = _make(name, max_batch=256)
    wt, table = R.nav_transform(name, w)
    assert list(w) == [k for k, _ in net.named_parameters()]
    states, B = _states(g), len(g["advs"])
    d = lambda k: torch.from_numpy(g[k]).cuda()

    def run(weights):
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in weights.items()})
        (_, logp), values = net(states, torch.from_numpy(g["actions"]))
        out = {"logp": logp.cpu().numpy().copy(), "value": values[0].cpu().numpy().copy()}
        net._ensure_packed()
        net._iter_chunk(net._stage(states, 0, B), B, d("actions"), d("old_logps"), d("advs"), d("rets"), B)
        flat = net.gtmp[:net.n_params + 3].cpu().numpy()
        out["losses"] = flat[net.n_params:].copy()
        off = 0
        for k, p in net.named_parameters():
            out["grad/" + k] = flat[off:off + p.numel()].copy()
            off += p.numel()
        return out

    base = run(w)
    got = run(wt)
    ex = {k: (table["grad"][k[5:]] if k.startswith("grad/") else 0) for k in base}
    assert all(np.isfinite(v).all() for v in base.values()) and all(np.abs(base["grad/" + k]).max() > 0 for k in w)
    bad = _mismatches(base, got, ex)
    assert not bad, "\n".join(bad)


# ---- float64 anchor ---------------------------------------------------------------------------------------------------------------
def _against_float64(h, weights, batch, tag):
    """ppo_iter on `weights`, then the per-tensor criterion of F3 / F21 against the float64 oracle under the kernels' leaky-ReLU
    decisions; the ratio to the fp32 oracle's own error is recorded under scale_invariance/<tag>."""
    frames, actions, old_logps, advs, rets = batch
    h.set_params(flatten(weights))
    h.ppo_iter(dev(frames), dev(actions), dev(old_logps), dev(advs), dev(rets))
    flat = h.grads.cpu().numpy()
    got = _views(flat[:h.n_params], False)
    o64 = P.oracle64_with_kernel_decisions(h, O.OraclePPO, weights, frames, actions, old_logps, advs, rets, with_fp32=True)
    np.testing.assert_allclose(flat[h.n_params:h.n_params + 3], o64.losses, rtol=2e-5, atol=2e-6)
    g32 = {k: p.grad.numpy() for k, p in o64.net32.named_parameters()}
    ratios, failed = {}, []
    for name, p in o64.net.named_parameters():
        want = p.grad.numpy()
        scale = np.abs(want).max()
        assert scale > 0, name
        err = np.abs(got[name] - want).max()
        a, b = got[name].astype(np.float64).ravel(), want.ravel()
        one_minus_cos = 1.0 - a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
        err32 = np.abs(g32[name] - want).max()
        ratios[name] = err / max(err32, 2.0 ** -24 * scale)     # an fp32 gradient is no closer than half a unit of its largest element
        print("%s %s: kernel %.2e max|g64| (1 - cos %.1e), fp32 oracle %.2e, ratio %.2f" % (
            tag, name, err / scale, one_minus_cos, err32 / scale, ratios[name]))
        if not (err <= 2e-5 * scale and one_minus_cos < 1e-9):
            failed.append((name, err / scale, one_minus_cos))
    P.MARGINS.record_vs_fp32_oracle("scale_invariance/" + tag, ratios)
    assert not failed, failed


def test_set_a_against_float64(hp):
    wt, _ = R.atari_transform(make_weights(0), R.SETS["A"])
    _against_float64(hp, wt, R.atari_batch(37), "set_A")


@pytest.mark.parametrize("below", [False, True], ids=["maximum_is_a_power_of_two", "maximum_is_just_below_one"])
def test_weight_maxima_at_the_ends_of_a_binade_against_float64(hp, below):
    """f16_scale puts a maximum into [2^12, 2^13) by frexpf: each encoder weight tensor's largest element is set to the power of two
    at or above it, or to the float just below that (the fp32 oracle alone is inside the criterion on both:
    tests/test_scale_invariance_cpu.py).  The planted element is the tensor's own largest, sign kept."""
    w, planted = R.binade_edge_weights(make_weights(0), below)
    assert len(planted) == 8
    _against_float64(hp, w, R.atari_batch(37), "binade_%s" % ("below" if below else "at"))
    pm = hp.plane_maxima()
    for name, (_, v) in planted.items():
        slot = {"conv1": "w1", "conv2": "w2", "conv3": "w3", "linear": "wl"}[name.split(".")[-2]]
        assert pm[slot][0 if name.startswith("actor") else 1] == np.float32(abs(v)), name
