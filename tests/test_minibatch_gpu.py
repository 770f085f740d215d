"""PPO minibatch epochs on the device: the four operators of csrc/minibatch.hip against numpy, and PPO.learn with the knobs of
nn/minibatch.py against the parent path's API driven by hand (tests/minibatch_ref.py hand_loop): the kernels are deterministic and the
gathered bytes are the same bytes, so losses, parameters and optimiser state are compared bit for bit.

Measured on an MI355X (recorded, not limits): moment sums within 2.4e-16 relative of numpy float64 (bound 1e-12); normalised columns at
most 0.48 of the derived bound; first-step losses of the normalised runs within 0.02 of the loss tolerance against the float64
oracle, the two-rank step within 0.01 of it."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import minibatch_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENT_F, SENT_B = -7.5e8, 0xA5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. moments -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def column(kind, n):
    rng = np.random.default_rng(1000 * n + len(kind))
    x = rng.normal(size=n)
    return ((0.3 + x) if kind == "near" else (1000.0 + x)).astype(np.float32)


@pytest.mark.parametrize("kind", ["near", "far"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_moments_against_float64(n, kind):
    from ddrl4nav_amd import ops
    x = column(kind, n)
    want = R.moments64(x)
    xd = dev(x)
    got = ops.moments(xd).cpu().tolist()
    print("moments n=%d %s: relative errors %s" % (n, kind, [abs(g - w) / abs(w) for g, w in zip(got, want)]))
    assert got[0] == float(n)
    for k in (1, 2):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    assert ops.moments(xd).cpu().tolist() == got                        # a repeat: the same bits
    # two halves accumulated (n = 1: the one sample on top of zeros)
    h = n // 2
    sums = torch.zeros(3, dtype=torch.float64, device="cuda")
    if h:
        ops.moments(xd[:h], sums=sums)
    two = ops.moments(xd[h:], sums=sums, accumulate=True).cpu().tolist()
    assert two[0] == float(n)
    for k in (1, 2):
        assert abs(two[k] - want[k]) <= 1e-12 * abs(want[k]), (k, two[k], want[k])


# ---- 2. affine and normalise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["near", "far", "constant"])
@pytest.mark.parametrize("n", [1, 2, 65, 4097])
@pytest.mark.parametrize("eps", [1e-8, 1e-3])
def test_normalise_against_float64(n, kind, eps):
    from ddrl4nav_amd import ops
    x = np.full(n, 0.7, np.float32) if kind == "constant" else column(kind, n)
    xd = dev(x)
    affine = ops.moments_affine(ops.moments(xd), eps)
    out = torch.full((n + 3,), SENT_F, dtype=torch.float32, device="cuda")
    ops.normalize(xd, affine, out=out, n=n)
    got = out.cpu().numpy()
    assert (got[n:] == np.float32(SENT_F)).all()
    r, bound = R.normalized64(x, eps)
    err = np.abs(got[:n].astype(np.float64) - r)
    print("normalise n=%d %s eps=%g: worst error / bound %.3f" % (n, kind, eps, float((err / bound).max())))
    assert (err <= bound).all(), float((err / bound).max())
    if n == 1 or kind == "constant":
        assert not got[:n].any()                                        # std 0 and numerator 0: zeros, not NaN
    a = affine.cpu().numpy()
    mean = x.astype(np.float64).mean()
    assert abs(float(a[0]) - mean) <= R.U * abs(mean) + 1e-12
    inplace = xd.clone()
    ops.normalize(inplace, affine, out=inplace)
    assert torch.equal(inplace, out[:n])                                # in place: the same bits


# ---- 3. the collation -------------------------------------------------------------------------------------------------------------------
N_ROWS = 9


@functools.lru_cache(maxsize=None)
def gather_source(C):
    rng = np.random.default_rng(40 + C)
    frames = rng.integers(0, 256, size=(N_ROWS, C, 84, 84), dtype=np.uint8)
    cols = rng.normal(size=(4, N_ROWS)).astype(np.float32)
    return frames, cols


def gather_indices(n):
    rng = np.random.default_rng(n)
    idx = rng.integers(0, N_ROWS, size=n).astype(np.int32)
    if n >= 5:
        idx[1], idx[3], idx[4] = -1, N_ROWS, idx[0]                     # below, past the end, a duplicate
    return idx


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("n", [1, 5, 37])
def test_gather_minibatch_against_fancy_indexing(C, n):
    from ddrl4nav_amd import ops
    frames, cols = gather_source(C)
    assert frames[0].size // 16 == 441 * C
    idx = gather_indices(n)
    ok = (idx >= 0) & (idx < N_ROWS)
    safe = np.where(ok, idx, 0)
    want_f = np.where(ok[:, None, None, None], frames[safe], 0).astype(np.uint8)
    want_c = np.where(ok[None, :], cols[:, safe], 0.0).astype(np.float32)
    fd, cd, idx_d = dev(frames), [dev(c) for c in cols], dev(idx)

    def run(affine=None):
        dst_f = torch.full((n + 1, C, 84, 84), SENT_B, dtype=torch.uint8, device="cuda")
        dst_c = [torch.full((n + 2,), SENT_F, dtype=torch.float32, device="cuda") for _ in range(4)]
        ops.gather_minibatch(fd, idx_d, dst_f, cd, dst_c, adv_affine=affine, n=n)
        torch.cuda.synchronize()
        assert bool((dst_f[n:] == SENT_B).all()) and all(bool((c[n:] == SENT_F).all()) for c in dst_c)      # nothing behind the ends
        return dst_f[:n], [c[:n] for c in dst_c]

    got_f, got_c = run()
    assert np.array_equal(got_f.cpu().numpy(), want_f)
    for k in range(4):
        assert got_c[k].cpu().numpy().tobytes() == want_c[k].tobytes(), k
    # the fused normalisation: bit-equal to ddrl_op_normalize of the plain gather (zeros of a bad index stay zeros)
    affine = dev(np.array([0.25, 1.75], np.float32))
    fused_f, fused_c = run(affine)
    assert torch.equal(fused_f, got_f)
    plain = ops.normalize(got_c[2], affine)
    plain = torch.where(dev(ok), plain, torch.zeros_like(plain))
    assert torch.equal(fused_c[2], plain)
    for k in (0, 1, 3):
        assert torch.equal(fused_c[k], got_c[k])
    # frames alone: the columns are optional
    only = torch.full((n + 1, C, 84, 84), SENT_B, dtype=torch.uint8, device="cuda")
    ops.gather_minibatch(fd, idx_d, only, n=n)
    assert torch.equal(only[:n], got_f) and bool((only[n:] == SENT_B).all())


# ---- 4. PPO.learn against the hand-composed loop ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(B, shared=0):
    """(batch, recipe weights) of config_cross.cell_inputs at C = 4, A = 6: computed once, never modified."""
    return R.batch_of(R.cell(B, shared))


def assert_same_run(items_a, items_b, net_a, net_b):
    assert len(items_a) == len(items_b)
    for (la, ua), (lb, ub) in zip(items_a, items_b):
        assert ua == ub
        assert {k: la[k] for k in R.LOSS_KEYS} == lb, (ua, la, lb)        # floats compared with ==: the same bits
    sa, sb = R.state_of(net_a), R.state_of(net_b)
    assert sa["step"] == sb["step"] and sa["update_time"] == sb["update_time"]
    for k in ("params", "m", "v"):
        assert np.array_equal(sa[k], sb[k]), k


def both(B, K, epochs, shuffle, shared=0, mode=None, eps=1e-8, **extra):
    """Net A through learn with the knobs, net B by hand; returns (items A, items B, net A, net B, the steps' indices)."""
    batch, w = problem(B, shared)
    knobs = dict(PPO_MINIBATCHES=K, PPO_SHUFFLE=shuffle, NORMALIZE_ADVANTAGE=mode or False, ADV_NORM_EPS=eps)
    net_a = R.make_net(w, B, shared, iters=epochs, **knobs, **extra)
    net_b = R.make_net(w, B, shared, iters=epochs)
    assert net_a.hot_path.max_batch == net_b.hot_path.max_batch == B
    steps = R.step_indices(net_a._seed, 0, epochs, B, K, shuffle)
    items_a = R.run_learn(net_a, batch)
    items_b = R.hand_loop(net_b, batch, steps, mode=mode, eps=eps)
    return items_a, items_b, net_a, net_b, steps


LEARN_CASES = {
    "B37-K3-2epochs-shuffled": dict(B=37, K=3, epochs=2, shuffle=True),
    "B37-K3-in-order": dict(B=37, K=3, epochs=1, shuffle=False),
    "B5-K5-single-samples": dict(B=5, K=5, epochs=1, shuffle=True),
    "shared-encoder-K2": dict(B=37, K=2, epochs=1, shuffle=True, shared=1),
}


@pytest.mark.parametrize("case", list(LEARN_CASES), ids=list(LEARN_CASES))
def test_learn_equals_the_hand_composed_loop(case):
    c = LEARN_CASES[case]
    items_a, items_b, net_a, net_b, steps = both(**c)
    assert len(items_a) == c["epochs"] * c["K"] and [u for _, u in items_a] == list(range(1, len(items_a) + 1))
    assert sorted(torch.cat(steps[:c["K"]]).tolist()) == list(range(c["B"]))      # an epoch visits every sample once
    assert_same_run(items_a, items_b, net_a, net_b)
    assert net_a.learn_calls == 1 and net_a.hot_path.max_batch == c["B"]


def test_defaults_take_the_parent_branch():
    """K = 1 with everything off: plain learn, against two full-batch steps by hand in storage order."""
    batch, w = problem(37)
    net_a, net_b = R.make_net(w, 37, iters=2), R.make_net(w, 37, iters=2)
    items_a = R.run_learn(net_a, batch)
    items_b = R.hand_loop(net_b, batch, [torch.arange(37)] * 2)
    assert_same_run(items_a, items_b, net_a, net_b)
    assert net_a.learn_calls == 0 and net_a._mb_stage is None               # the minibatch loop was never entered


def test_more_minibatches_than_samples_is_refused_at_learn():
    batch, w = problem(5)
    net = R.make_net(w, 5, PPO_MINIBATCHES=6)
    with pytest.raises(ValueError, match="PPO_MINIBATCHES"):
        next(net.learn(R.experience(batch)))
    assert net.update_time == 0


def test_capacity_is_ensured_for_the_largest_minibatch_only():
    batch, w = problem(37)
    net = R.make_net(w, 8, PPO_MINIBATCHES=3)
    assert len(R.run_learn(net, batch)) == 3
    assert net.hot_path.max_batch == 13


def test_deferred_readback_yields_the_eager_rows():
    batch, w = problem(37)
    items_e, items_b, net_e, net_b, _ = both(37, 3, 2, True)
    net_d = R.make_net(w, 37, iters=2, PPO_MINIBATCHES=3, PPO_SHUFFLE=True, DEFERRED_LOSS_READBACK=True)
    items_d = R.run_learn(net_d, batch)
    assert len(items_d) == 6 and net_d._stats_rows.shape[0] >= 6
    assert_same_run(items_d, items_b, net_d, net_b)
    assert items_d == items_e


def test_target_kl_ends_the_call_at_the_step_that_trips():
    """A target between the first two steps' KL: step 2 is evaluated and not applied, exactly one yield, parameters as after one step.
    The batch's old log-probs are off the policy from the start, so which configuration has a second minibatch further off than the
    first is looked up with a diagnostics run."""
    batch, w = problem(37)
    for K, shuffle in ((3, False), (3, True), (2, False), (2, True), (4, False), (4, True)):
        net = R.make_net(w, 37, PPO_MINIBATCHES=K, PPO_SHUFFLE=shuffle, PPO_DIAGNOSTICS=True)
        kl = [ld["ApproxKL"] for ld, _ in R.run_learn(net, batch)]
        if kl[1] > 1.01 * kl[0] > 0:
            break
    else:
        raise AssertionError("no configuration whose second step's KL exceeds the first's")
    target = float(np.sqrt(kl[0] * kl[1])) / 1.5
    net_a = R.make_net(w, 37, iters=2, PPO_MINIBATCHES=K, PPO_SHUFFLE=shuffle, TARGET_KL=target)
    net_b = R.make_net(w, 37)
    items_a = R.run_learn(net_a, batch)
    assert len(items_a) == 1 and items_a[0][1] == 1 and items_a[0][0]["ApproxKL"] == kl[0]
    items_b = R.hand_loop(net_b, batch, R.step_indices(net_a._seed, 0, 1, 37, K, shuffle), max_steps=1)
    assert_same_run(items_a, items_b, net_a, net_b)


@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffled", "in-order"])
@pytest.mark.parametrize("mode", ["batch", "minibatch"])
def test_normalised_advantages(mode, shuffle):
    B, K, eps = 37, 3, 1e-8
    batch, w = problem(B)
    items_a, items_b, net_a, net_b, steps = both(B, K, 1, shuffle, mode=mode, eps=eps)
    assert_same_run(items_a, items_b, net_a, net_b)
    # independently: the first step against the float64 oracle on float64-normalised advantages
    sel = steps[0].numpy()
    adv64, _ = R.normalized64(batch["advs"][sel], eps, pool=batch["advs"] if mode == "batch" else None)
    want = R.oracle_losses64(w, batch, sel, adv64)
    got = [items_a[0][0][k] for k in ("ActorLoss", "VLoss", "EntLoss")]
    print("normalised %s: losses %s, oracle %s" % (mode, got, want))
    np.testing.assert_allclose(got, want, **R.LOSS_TOL)
    raw = [R.hand_loop(R.make_net(w, B), batch, steps, max_steps=1)[0][0][k] for k in ("ActorLoss",)]
    assert raw[0] != got[0]                                               # the knob did something


# ---- 5. two ranks -----------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_share_the_moments_and_stay_in_step(tmp_path):
    """Shards of 20 and 17 samples on two gloo ranks sharing the GPU, K = 2, shuffled, "batch" normalisation."""
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.engine import HotPath
    from ddrl4nav_amd.utils.recipe import flatten
    batch, w = problem(37)
    np.savez(tmp_path / "batch.npz", **batch)
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   DDRL_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "minibatch_worker.py"), str(tmp_path),
                                       str(tmp_path / "batch.npz"), "0,20,37"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True))
    try:
        for r, p in enumerate(procs):      # the first failure ends the test (and the other rank)
            out, _ = p.communicate(timeout=300)
            assert p.returncode == 0, "rank %d failed (%d):\n%s" % (r, p.returncode, out[-3000:])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(2))
    for k in ("params", "m", "v", "affine", "losses"):
        assert np.array_equal(r0[k], r1[k]), k
    assert int(r0["yields"]) == int(r1["yields"]) == 2 and int(r0["step"]) == int(r1["step"]) == 2
    # the first step on one process: both ranks' first minibatches, advantages normalised over all 37 samples
    sel = np.concatenate([r0["first"], 20 + r1["first"]])
    assert len(sel) == 10 + 9 and len(set(sel.tolist())) == 19
    affine = ops.moments_affine(ops.moments(dev(batch["advs"])), 1e-8)
    assert np.array_equal(affine.cpu().numpy(), r0["affine"])
    adv = ops.normalize(dev(batch["advs"]), affine)[dev(sel)].contiguous()
    hp = HotPath(max_batch=37)
    hp.set_params(flatten(w))
    hp.ppo_iter(dev(batch["frames"][sel]), dev(batch["actions"][sel]), dev(batch["old_logps"][sel]), adv, dev(batch["rets"][sel]))
    s = hp.stats()
    hp.close()
    one = [s[k] for k in ("ActorLoss", "VLoss", "EntLoss")]
    print("two ranks: first-step losses %s, one process %s" % (r0["losses"][0].tolist(), one))
    np.testing.assert_allclose(r0["losses"][0], one, **R.LOSS_TOL)
