"""The PPO update diagnostics on the device (csrc/diag.hip; include/ddrl.h ddrl_op_heads_diag / ddrl_ppo_diag) and what is built on
them: ApproxKL / ClipFraction / ExplainedVariance / RatioMax in the loss dicts of PPO.learn and KL early stopping.

Operator level: both head families against the float64 reference of tests/ppo_diag_ref.py, with the tolerances of the eight sums
propagated from the project's own log-prob / value tolerance; the clipped COUNT exactly (the recipe keeps every
ratio 0.1 from 1 +- clip; tests/test_ppo_diag_cpu.py checks that on the reference's own fp32 run).  The measured slack (error / bound,
worst case per slot) is written to the file DDRL_DIAG_MARGINS_OUT names, when it is set; tests/golden/ppo_diag_margins.json is a
copy of one such run -- a record, not a limit."""
import json
import os
import socket
import subprocess
import sys
import types
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

import heads_ref as H
import ppo_diag_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENT = -7.5e8          # what the optional outputs hold where the kernel must not write
SUM_SLOTS, EXACT_SLOTS = (1, 3, 4, 5, 6), (0, 2, 7)
_SLACK = {}


def _note(slot, err, bound):
    if bound > 0:
        _SLACK[slot] = max(_SLACK.get(slot, 0.0), err / bound)


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    path = os.environ.get("DDRL_DIAG_MARGINS_OUT")
    if _SLACK and path:
        with open(path, "w") as f:
            json.dump({"what": "worst error / bound per checked quantity, tests/test_ppo_diag_gpu.py", "slack": _SLACK}, f, indent=1,
                      sort_keys=True)


def _carve(low, high):
    """Device copies of two host tensors inside ONE allocation, `low` at the lower address."""
    buf = torch.cat([low.reshape(-1), high.reshape(-1)]).cuda()
    return buf[:low.numel()].view(low.shape), buf[low.numel():].view(high.shape)


def run_diag(c, below=False, old_logps=None, parts=None):
    """ddrl_op_heads_diag on a case of heads_ref: one call, or one call per (lo, hi) of `parts` accumulating into the same sums."""
    from ddrl4nav_amd import _lib, ops
    L = H.head_layout(c.continuous, c.A)
    d = _lib.HeadsDesc(1 if c.continuous else 0, c.A, 1 if c.shared else 0, 0, L["actor_w"], L["actor_b"], L["log_std"], L["critic_w"],
                       L["critic_b"], L["n_params"])
    cfg = _lib.default_config(max_batch=max(c.n, 8), n_actions=max(2, min(c.A, 18)), ppo_clip=c.hyper["ppo_clip"])
    params = H.fill_arena(L, c.params, fill=0.5).cuda()       # finite junk between the slots: nothing may read it into a result
    ha, hc = c.ha.cuda(), c.hc.cuda()
    if below:      # the critic's features at LOWER addresses than the actor's: a negative stride in the kernel
        hc, ha = _carve(c.hc, c.ha)
        assert hc.data_ptr() < ha.data_ptr()
    acts, rets = c.actions.contiguous().cuda(), c.rets.contiguous().cuda()
    old = (c.old_logps if old_logps is None else old_logps).contiguous().cuda()
    logp = torch.full((c.n + 2,), SENT, dtype=torch.float32, device="cuda")
    value = torch.full((c.n + 2,), SENT, dtype=torch.float32, device="cuda")
    sums = None
    for i, (lo, hi) in enumerate(parts or [(0, c.n)]):
        sums = ops.heads_diag(d, cfg, params, ha[lo:hi], hc[lo:hi], hi - lo, acts[lo:hi], old[lo:hi], rets[lo:hi], sums=sums,
                              accumulate=i > 0, logp_out=logp[lo:hi], value_out=value[lo:hi])
    torch.cuda.synchronize()
    assert bool((logp[c.n:] == SENT).all()) and bool((value[c.n:] == SENT).all())
    return sums.cpu().tolist(), logp[:c.n].cpu(), value[:c.n].cpu()


def check_against_reference(c, got, tag):
    sums, logp, value = got
    ref = R.reference(c)
    el = (logp.double() - ref["logp"]).abs()
    ev = (value.double() - ref["value"]).abs()
    _note("logp", float((el / ref["tau"]).max()), 1.0)
    _note("value", float((ev / ref["sigma"]).max()), 1.0)
    assert bool((el <= ref["tau"]).all()), (tag, float((el / ref["tau"]).max()))
    assert bool((ev <= ref["sigma"]).all()), (tag, float((ev / ref["sigma"]).max()))
    for k in range(8):
        err, bound = abs(sums[k] - ref["sums"][k]), ref["bounds"][k]
        _note("slot%d" % k, err, bound)
        assert err <= bound, (tag, k, sums[k], ref["sums"][k], err, bound)
    for k in (1, 2, 4, 6):
        assert sums[k] >= 0.0, (tag, k, sums[k])
    return ref


# ---- 1. the operator against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cont,A,shared,below", R.GRID, ids=[R.case_id(*g) for g in R.GRID])
def test_sums_and_per_sample_outputs_against_float64(cont, A, shared, below):
    for n in R.NS:
        c = R.make_case(cont, A, n, shared)
        check_against_reference(c, run_diag(c, below=below), "%s n=%d" % (R.case_id(cont, A, shared, below), n))


def test_explained_variance_survives_returns_far_from_zero():
    """Returns with mean 20 and std 0.05: sum(ret^2) / n - mean^2 loses 5 of the 7 digits an fp32 sum has, so an fp32 sum of squares
    gives an explained variance of the wrong size; the double sums keep it inside what the slot bounds allow."""
    from ddrl4nav_amd import ops
    g = torch.Generator().manual_seed(77)
    rets = (20.0 + 0.05 * torch.randn(1025, generator=g, dtype=torch.float64)).float()
    for cont, A in ((0, 6), (1, 2)):
        c = R.make_case(cont, A, 1025, False, rets=rets)
        got = run_diag(c)
        ref = check_against_reference(c, got, "cancellation")
        bound, want = R.explained_variance_bound(ref)
        ev = ops.diag_dict(got[0])["ExplainedVariance"]
        _note("explained_variance_cancellation", abs(ev - want), bound)
        assert abs(ev - want) <= bound, (ev, want, bound)
        # what the test is about: the same quantity from an fp32 sum of squares misses that bound
        s32 = list(ref["sums"])
        s32[4] = float((c.rets * c.rets).sum(dtype=torch.float32))
        assert abs(ops.diag_dict(s32)["ExplainedVariance"] - want) > bound


def test_accumulate_builds_the_whole_from_two_calls():
    for cont, A, shared in ((0, 6, False), (0, 18, True), (1, 8, False)):
        c = R.make_case(cont, A, 1025, shared)
        whole = run_diag(c)
        halves = run_diag(c, parts=[(0, 257), (257, 1025)])
        for k in SUM_SLOTS:
            assert abs(halves[0][k] - whole[0][k]) <= 1e-12 * abs(whole[0][k]), (k, halves[0][k], whole[0][k])
        for k in EXACT_SLOTS:
            assert halves[0][k] == whole[0][k], k
        assert torch.equal(halves[1], whole[1]) and torch.equal(halves[2], whole[2])      # the per-sample outputs do not depend on the split


def test_a_policy_against_itself_has_no_divergence():
    """old_logps := the log-probs of a first call: every x is 0 exactly, so KL sum 0, nothing clipped, largest ratio 1."""
    for cont, A, shared in ((0, 2, False), (0, 6, True), (0, 18, False), (1, 1, False), (1, 8, True)):
        for n in (5, 1025):
            c = R.make_case(cont, A, n, shared)
            _, logp, _ = run_diag(c)
            sums, logp2, _ = run_diag(c, old_logps=logp)
            assert torch.equal(logp, logp2)
            assert sums[0] == float(n) and sums[1] == 0.0 and sums[2] == 0.0 and sums[7] == 1.0, sums


def test_argument_checks_come_before_any_launch():
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    L = H.head_layout(0, 6)
    d = _lib.HeadsDesc(0, 6, 0, 0, L["actor_w"], L["actor_b"], 0, L["critic_w"], L["critic_b"], L["n_params"])
    cfg = _lib.default_config(max_batch=8)
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    base = buf.data_ptr()
    a, st = c_void_p(base), c_void_p(0)
    w, s8 = c_void_p(base + 4 * 32768), c_void_p(base + 4 * 60000)      # 16,384 floats of scratch and the 8 doubles: apart from what is read
    odd, null = c_void_p(base + 4), c_void_p(0)

    def call(desc=d, params=a, ha=a, hc=a, n=4, acts=a, sums=s8, ws=w):
        return lib.ddrl_op_heads_diag(byref(desc), byref(cfg), params, ha, hc, n, acts, a, a, sums, 0, null, null, ws, st)

    assert call() == 0
    bad = _lib.HeadsDesc(0, 19, 0, 0, L["actor_w"], L["actor_b"], 0, L["critic_w"], L["critic_b"], L["n_params"])
    for kw in (dict(desc=bad), dict(params=null), dict(ha=null), dict(hc=null), dict(n=0), dict(acts=null), dict(sums=null), dict(ws=null),
               dict(ha=odd), dict(hc=odd), dict(ws=odd), dict(sums=odd)):
        assert call(**kw) == -1, kw
    shared = _lib.HeadsDesc(0, 6, 1, 0, L["actor_w"], L["actor_b"], 0, L["critic_w"], L["critic_b"], L["n_params"])
    assert call(desc=shared, hc=null) == 0          # a shared prenet does not read h_critic
    torch.cuda.synchronize()


# ---- 2. the Atari context ----------------------------------------------------------------------------------------------------------------
def _atari_batch(seed=3, B=64):
    """B random frames, the actions the net samples on them, its own log-probs as old_logps (ratios start at 1 up to the rounding
    between the acting and the training forward), advantages N(0, 1), returns = value + N(0, 0.5)."""
    from ddrl4nav_amd.engine import HotPath
    from ddrl4nav_amd.utils.recipe import flatten, make_weights
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(B, 4, 84, 84), dtype=np.uint8)
    hp = HotPath(max_batch=B)
    hp.set_params(flatten(make_weights(0)))
    _, value, action, logp = hp.forward(torch.from_numpy(frames).cuda(), seed=11, stream_id=1)
    out = {"frames": frames, "actions": action.cpu().numpy(), "old_logps": logp.cpu().numpy(),
           "advs": rng.normal(size=B).astype(np.float32),
           "rets": (value.cpu().numpy() + 0.5 * rng.normal(size=B)).astype(np.float32)}
    hp.close()
    return out


@pytest.fixture(scope="module")
def atari_batch():
    return _atari_batch()


def test_context_diag_equals_the_operator_and_leaves_the_update_alone(atari_batch):
    from ddrl4nav_amd import _lib, ops
    from ddrl4nav_amd.engine import HotPath
    from ddrl4nav_amd.utils.recipe import flatten, make_weights, param_specs
    b = atari_batch
    d = lambda k: torch.from_numpy(np.ascontiguousarray(b[k])).cuda()
    args = (d("frames"), d("actions"), d("old_logps"), d("advs"), d("rets"))
    runs = []
    for with_diag in (True, False):
        hp = HotPath(max_batch=64)
        hp.set_params(flatten(make_weights(0)))
        hp.ppo_iter(*args)
        if with_diag:
            sums = hp.ppo_diag(args[1], args[2], args[4]).cpu().tolist()
            ha, hc = hp.last_features(64)
            off, o = {}, 0
            for name, shape, _ in param_specs():
                off[name] = o
                o += int(np.prod(shape))
            desc = _lib.HeadsDesc(0, 6, 0, 0, off["actor.actor_linear.weight"], off["actor.actor_linear.bias"], 0,
                                  off["critic.critic_linear.weight"], off["critic.critic_linear.bias"], hp.n_params)
            want = ops.heads_diag(desc, hp.cfg, hp.params, ha, hc, 64, args[1], args[2], args[4]).cpu().tolist()
            for k in SUM_SLOTS:
                assert abs(sums[k] - want[k]) <= 1e-12 * abs(want[k]), (k, sums[k], want[k])
            for k in EXACT_SLOTS:
                assert sums[k] == want[k], k
            assert sums[0] == 64.0 and all(np.isfinite(sums))
            # another batch size, or features another forward has replaced: refused
            assert hp.lib.ddrl_ppo_diag(hp.ctx, c_void_p(args[1].data_ptr()), c_void_p(args[2].data_ptr()), c_void_p(args[4].data_ptr()),
                                        32, c_void_p(hp._diag_sums.data_ptr()), c_void_p(0)) == -1
        g_before = hp.grads.clone()
        hp.clip_adam_step()
        runs.append((g_before.cpu(), hp.grads.cpu().clone(), hp.params.cpu().clone()))
        if with_diag:
            hp.forward(args[0][:8])
            with pytest.raises(_lib.DdrlError):
                hp.ppo_diag(args[1], args[2], args[4])
        hp.close()
    for x, y in zip(*runs):
        assert torch.equal(x, y)       # gradient arena + statistics tail (before and after the step) and the parameters: bit-identical


# ---- 3. PPO.learn ------------------------------------------------------------------------------------------------------------------------
DIAG_KEYS = ("ApproxKL", "ClipFraction", "ExplainedVariance", "RatioMax")
TODAY_KEYS = {"PpoTotalLoss", "ActorLoss", "VLoss", "EntLoss", "PpoBackUpTime"}


def run_learn(batch, lo=0, hi=None, iters=4, lr_scale=1.0, **options):
    """create_net -> PPO.learn on samples [lo, hi) of the batch with config_nn options set by name; what every yield carried, the
    parameters after it, the combined raw sums of every diagnosed iteration.  (tests/ppo_diag_worker.py runs this per rank.)"""
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.data import Experience
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.utils.recipe import make_weights
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": 4, "discrete_action": True,
           "discrete_actions": list(range(6)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg_nn = ConfigNN(env)
    cfg_nn.TRAINING_ITER_TIME = iters
    cfg_nn.ACTOR_LEARNING_RATE = cfg_nn.ACTOR_LEARNING_RATE * lr_scale
    for k, v in options.items():
        setattr(cfg_nn, k, v)
    net = create_net({"config": BaseConfig(types.SimpleNamespace(task="diag", ip="127.0.0.1"), env), "config_nn": cfg_nn,
                      "config_env": env}, max_batch=64)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_weights(0).items()})
    hi = len(batch["actions"]) if hi is None else hi
    exp = Experience(states=[batch["frames"][lo:hi]], advs=batch["advs"][lo:hi], actions=batch["actions"][lo:hi],
                     old_logps=batch["old_logps"][lo:hi], values=batch["rets"][lo:hi].reshape(1, -1))
    exp.to_tensor(dtype=torch.float32, device="cuda")
    raw = []
    hp = net.hot_path
    combine = hp.diag_global
    hp.diag_global = lambda s: (raw.append(combine(s)), raw[-1])[1]
    out = {"items": [], "params": [], "diag": []}
    for it, (ld, update_time, last) in enumerate(net.learn(exp), 1):
        assert update_time == it and last is True
        out["items"].append(dict(ld))
        out["params"].append(hp.params.cpu().numpy().copy())
        if "ApproxKL" in ld:
            out["diag"].append([ld[k] for k in DIAG_KEYS])
    out["raw_sums"] = raw
    out["update_time"] = net.update_time
    out["final_params"] = hp.params.cpu().numpy().copy()
    hp.close()
    return out


@pytest.fixture(scope="module")
def learn_runs(atari_batch):
    """One run with the diagnostics, one without; the learning rate is raised until the KL grows fourfold between two iterations
    (the early-stopping test needs such a step)."""
    for lr_scale in (1.0, 10.0, 100.0):
        on = run_learn(atari_batch, lr_scale=lr_scale, PPO_DIAGNOSTICS=True)
        kl = [d[0] for d in on["diag"]]
        ks = [k for k in range(1, len(kl)) if kl[k - 1] > 0 and kl[k] >= 4 * kl[k - 1]]
        if ks:
            return {"on": on, "off": run_learn(atari_batch, lr_scale=lr_scale), "k": ks[0], "kl": kl, "lr_scale": lr_scale}
    raise AssertionError("no fourfold KL step at any learning rate: %r" % (kl,))


def test_learn_reports_the_diagnostics_and_changes_nothing_else(atari_batch, learn_runs):
    on, off = learn_runs["on"], learn_runs["off"]
    assert len(on["items"]) == len(off["items"]) == 4
    for a, b, pa, pb in zip(on["items"], off["items"], on["params"], off["params"]):
        assert set(b) == TODAY_KEYS and set(a) == TODAY_KEYS | set(DIAG_KEYS)
        assert all(np.isfinite(a[k]) for k in DIAG_KEYS)
        assert 0.0 <= a["ClipFraction"] <= 1.0 and a["ApproxKL"] >= 0.0 and a["RatioMax"] > 0.0
        assert all(a[k] == b[k] for k in TODAY_KEYS - {"PpoBackUpTime"})
        assert np.array_equal(pa, pb)                       # the parameters after every yield: bit-identical to the run without
    # the first iteration sees the collecting policy itself: ratios are 1 up to the rounding between two forward kernels
    assert on["diag"][0][0] < 1e-8 and on["diag"][0][1] == 0.0 and abs(on["diag"][0][3] - 1.0) < 1e-3
    deferred = run_learn(atari_batch, lr_scale=learn_runs["lr_scale"], PPO_DIAGNOSTICS=True, DEFERRED_LOSS_READBACK=True)
    assert deferred["diag"] == on["diag"]                   # the same four numbers, bit for bit
    assert np.array_equal(deferred["final_params"], on["final_params"])


def _target_between(kl, k):
    """TARGET_KL such that 1.5 x TARGET_KL is the geometric mean of KL_k and KL_{k+1} (1-based)."""
    return float(np.sqrt(kl[k - 1] * kl[k])) / 1.5


def test_target_kl_stops_before_the_step_that_went_too_far(atari_batch, learn_runs):
    k, kl, on = learn_runs["k"], learn_runs["kl"], learn_runs["on"]
    run = run_learn(atari_batch, lr_scale=learn_runs["lr_scale"], TARGET_KL=_target_between(kl, k))
    assert len(run["items"]) == k and run["update_time"] == k
    assert [d[0] for d in run["diag"]] == kl[:k]
    assert np.array_equal(run["final_params"], on["params"][k - 1])      # iteration k + 1 was evaluated, not applied
    assert set(run["items"][0]) == TODAY_KEYS | set(DIAG_KEYS)            # a target implies the diagnostics


# ---- 4. two ranks ------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_report_and_decide_alike(tmp_path, atari_batch, learn_runs):
    """Uneven shards (40 + 24) on two gloo ranks sharing the GPU: the ranks' sums are combined before anyone looks, so both report
    the same bits and stop at the same iteration; at the first iteration -- the same weights as the one-rank run -- the combined
    sums are the one-rank sums (later iterations follow all-reduced gradients, whose rounding differs from one rank's)."""
    k, kl = learn_runs["k"], learn_runs["kl"]
    np.savez(tmp_path / "batch.npz", **atari_batch)
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   DDRL_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "ppo_diag_worker.py"), str(tmp_path), str(tmp_path / "batch.npz"),
                                       "0,40,64", repr(_target_between(kl, k)), repr(learn_runs["lr_scale"])], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, logs[r][-3000:])
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(2))
    assert r0["diag"].shape == (4, 4) and np.array_equal(r0["diag"], r1["diag"]) and np.array_equal(r0["raw_sums"], r1["raw_sums"])
    assert np.array_equal(r0["params"], r1["params"])
    one, two = learn_runs["on"]["raw_sums"][0], r0["raw_sums"][0]
    for s in SUM_SLOTS:
        assert abs(two[s] - one[s]) <= 1e-12 * abs(one[s]), (s, two[s], one[s])
    for s in EXACT_SLOTS:
        assert two[s] == one[s], s
    assert int(r0["stop_yields"]) == int(r1["stop_yields"]) == k
    assert int(r0["stop_update_time"]) == int(r1["stop_update_time"]) == k
    assert np.array_equal(r0["stop_params"], r1["stop_params"])
