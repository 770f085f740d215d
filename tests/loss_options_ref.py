"""What tests/test_loss_options_*.py share: the PPO update options (clipped value loss, split-net entropy bonus,
annealed rates) restated in plain torch / Python.  heads_ref.make_case extended by the fifth column (old_values), the loss block of
heads_ref.loss_block with the options (torch.max / torch.clamp: autograd supplies the tie and closed-interval conventions), the float64
oracle of the whole Atari context under the options, and the hand-driven loops the learn tests compare against.  Nothing at import
time needs a GPU."""
import os
import re

import numpy as np
import torch

import heads_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VALUE_CLIP = 0.4                                   # c of the cases below
D_OVER_C = (-3.0, -1.5, -0.5, 0.0, 0.5, 1.5, 3.0)   # (v - v_old) / c
CLIP_OUTCOMES = ("inside", "clipped_unclipped_larger", "clipped_clipped_larger", "tie")
OPTION_SETS = {"clip": (VALUE_CLIP, False), "entropy": (0.0, True), "both": (VALUE_CLIP, True)}


def d_index(i):
    """Position of sample i in D_OVER_C.  heads_ref places the returns with the seven-step cycle HUBER_E[i % 7]; this cycle has seven steps
    too, so it advances by one more step per seven samples: period 49, every (return distance, d / c) pair once in 49 samples."""
    return (i + i // 7) % 7


def make_case(continuous, A, n, shared, smooth, options, hyper=None, seed=0, B_global=None):
    """heads_ref.make_case plus c.value_clip, c.entropy_split and c.old_values = fp32(v64 - d), d / c cycling through D_OVER_C."""
    return attach_options(H.make_case(continuous, A, n, shared, smooth, hyper, seed=seed, B_global=B_global), options)


def attach_options(c, options):
    """The option fields and the fifth column on a finished case of heads_ref (make_case or make_peaked_case)."""
    c.value_clip, c.entropy_split = float(options[0]), bool(options[1])
    v64 = c.rets.double() - c.err64
    c.d_over_c = torch.tensor([D_OVER_C[d_index(i)] for i in range(c.n)], dtype=torch.float64)
    c.old_values = (v64 - c.d_over_c * VALUE_CLIP).float()
    c.v64 = v64
    return c


def element(x, smooth):
    """e(x): the value-loss element, x^2 / 2 or smooth-L1 with beta 1."""
    if smooth:
        ax = x.abs()
        return torch.where(ax < 1.0, 0.5 * x ** 2, ax - 0.5)
    return x ** 2 / 2


def clip_terms64(c):
    """(d, L_u, L_c, ret - v_c) of the case in float64, with the case's own clip constant VALUE_CLIP."""
    ret, old = c.rets.double(), c.old_values.double()
    d = c.v64 - old
    v_c = old + torch.clamp(d, -VALUE_CLIP, VALUE_CLIP)
    return d, element(ret - c.v64, c.smooth), element(ret - v_c, c.smooth), ret - v_c


def clip_outcomes(c):
    d, l_u, l_c, _ = clip_terms64(c)
    out = []
    for i in range(c.n):
        if float(c.d_over_c[i]) == 0.0:
            out.append("tie")
        elif abs(float(d[i])) <= VALUE_CLIP:
            out.append("inside")
        else:
            out.append("clipped_unclipped_larger" if float(l_u[i]) > float(l_c[i]) else "clipped_clipped_larger")
    return out


def check_recipe(c):
    """heads_ref.check_recipe and the fifth column's own promises, in float64: every | |d| - c | above 1e-3 (the fp32 difference a kernel
    forms lands on the same side of the clamp), every clipped sample's two elements more than 1e-4 apart (the same maximum), with
    smooth-L1 no |ret - v_c| within 1e-3 of 1, and from 64 samples up all four outcomes."""
    H.check_recipe(c)
    check_clip_recipe(c)


def check_clip_recipe(c):
    """The fifth column's promises alone (check_recipe; the peaked cases check theirs with heads_ref.check_peaked_recipe)."""
    d, l_u, l_c, err_c = clip_terms64(c)
    assert torch.isfinite(c.old_values).all()
    assert float(((d.abs() - VALUE_CLIP).abs()).min()) > 1e-3, float(((d.abs() - VALUE_CLIP).abs()).min())
    clipped = d.abs() > VALUE_CLIP
    if bool(clipped.any()):
        assert float((l_u - l_c).abs()[clipped].min()) > 1e-4, float((l_u - l_c).abs()[clipped].min())
    if c.smooth:
        assert float(((err_c.abs() - 1.0).abs()).min()) > 1e-3, float(((err_c.abs() - 1.0).abs()).min())
    # samples placed at d = 0 stay within rounding of it, samples placed inside stay inside
    assert float(d[c.d_over_c == 0].abs().max() if bool((c.d_over_c == 0).any()) else 0.0) < 1e-5
    if c.n >= 64:
        assert set(clip_outcomes(c)) == set(CLIP_OUTCOMES), sorted(set(clip_outcomes(c)))


def loss_block(c, dtype):
    """heads_ref.loss_block with the options of the case (c.value_clip 0 = off, c.entropy_split): the same outputs."""
    h = c.hyper
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in c.params.items()}
    ha = c.ha.to(dtype).clone().requires_grad_(True)
    hc = ha if c.shared else c.hc.to(dtype).clone().requires_grad_(True)
    dist, logp, ent_el, v, _ = H.forward(c, ha, hc, P, dtype)
    adv, old, ret = c.advs.to(dtype), c.old_logps.to(dtype), c.rets.to(dtype)
    ratio = torch.exp(logp - old)
    m = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - h["ppo_clip"], 1.0 + h["ppo_clip"]) * adv)
    term = torch.where(adv > 0, m, torch.max(m, h["dual_clip"] * adv))
    v_el = element(ret - v, c.smooth)
    if c.value_clip > 0:
        v_old = c.old_values.to(dtype)
        v_c = v_old + torch.clamp(v - v_old, -c.value_clip, c.value_clip)
        v_el = torch.max(v_el, element(ret - v_c, c.smooth))
    s = c.n / float(c.B_global)
    actor_loss, v_loss, ent = -term.mean() * s, v_el.mean() * s, ent_el.mean() * s
    if c.shared:
        (actor_loss + h["v_loss_theta"] * v_loss - h["ent_loss_theta"] * ent).backward()
    else:
        ((actor_loss - h["ent_loss_theta"] * ent) if c.entropy_split else actor_loss).backward(retain_graph=True)
        v_loss.backward()
    out = {"dist": dist.detach(), "logp": logp.detach(), "value": v.detach(), "dh_actor": ha.grad,
           "dh_critic": None if c.shared else hc.grad, "losses": torch.stack([actor_loss, v_loss, ent]).detach()}
    for k, p in P.items():
        out["g_" + k] = p.grad
    return {k: (None if t is None else t.detach().double()) for k, t in out.items()}


# ---- the grid of the operator test -------------------------------------------------------------------------------------------------------
def _const(path, name):
    src = open(os.path.join(ROOT, "ddrl4nav_amd", "csrc", path)).read()
    m = re.search(r"constexpr int [^;]*\b%s = (\d+)" % name, src)
    assert m, (path, name)
    return int(m.group(1))


def full_pass(continuous, A):
    """Samples one pass of the loss grid takes, read from the code: HEAD_WG workgroups x waves x samples per wave and turn."""
    wg = _const("common.h", "HEAD_WG")
    if continuous:    # gauss_loss_kernel: __launch_bounds__(256) = four waves, one sample per wave and turn
        src = open(os.path.join(ROOT, "ddrl4nav_amd", "csrc", "gheads.hip")).read()
        m = re.search(r"__launch_bounds__\((\d+)\) void gauss_loss_kernel", src)
        assert m
        return wg * (int(m.group(1)) // 64)
    waves = _const("heads.hip", "LOSS_WAVES6") if A <= 6 else _const("heads.hip", "LOSS_WAVES")
    return wg * waves * _const("heads.hip", "LOSS_NS")


def loss_cases():
    """(continuous, A, n, shared, smooth, option set, B_global): Categorical A = 6, 8, 18 (the three kernel classes) and Gaussian D = 2, 8;
    n = 1, 3, 5, 67 and one full pass of the grid plus a ragged tail of three; both sharing modes, both value losses and the three
    option sets spread over them (every (family, option set) meets both sharing modes and both value losses)."""
    cases = []
    for cont, sizes in ((0, (6, 8, 18)), (1, (2, 8))):
        for j, A in enumerate(sizes):
            for i, n in enumerate((1, 3, 5, 67, full_pass(cont, A) + 3)):
                for k, name in enumerate(("clip", "entropy", "both")):
                    shared, smooth = (i + j + k) % 2, ((i + j + k) // 2 + k) % 2
                    if n > 67 and name == "entropy" and A != sizes[0]:
                        continue              # the large batch once per family for the option that adds no load
                    cases.append((cont, A, n, shared, smooth, name, n if (i + k) % 2 else 3 * n + 1))
    return cases


def case_of(spec):
    cont, A, n, shared, smooth, name, B = spec
    return make_case(cont, A, n, shared, smooth, OPTION_SETS[name], seed=2, B_global=B)


def case_id(spec):
    cont, A, n, shared, smooth, name, B = spec
    return "%s%d-n%d-%s-%s-%s-B%d" % ("gauss" if cont else "cat", A, n, "shared" if shared else "split", "huber" if smooth else "mse", name, B)


# ---- annealing ------------------------------------------------------------------------------------------------------------------------------
def anneal_factor(u, n, floor=0.0):
    """s = max(f, 1 - u / N), in double."""
    return max(float(floor), 1.0 - float(u) / float(n))


def annealed_rates32(base, u, n, floor=0.0, clip_too=False):
    """The four fp32 numbers the context holds in front of step u: each product formed in double and rounded once."""
    s = anneal_factor(u, n, floor)
    out = [np.float32(float(b) * s) for b in base[:3]]
    out.append(np.float32(float(base[3]) * s) if clip_too else np.float32(base[3]))
    return [float(x) for x in out]


# ---- the whole Atari context against float64 -------------------------------------------------------------------------------------------------
def atari_losses(net, x, actions, old_logps, advs, rets, old_values, smooth_l1, value_clip):
    """oracle.ppo_losses with the clipped value loss (value_clip 0: its own expressions): (actor_loss, v_loss, entropy)."""
    from oracle import ddrl_oracle as O
    _, p_hat, logits, v = net(x)
    # the oracle clamps with the eps of its OWN dtype (torch.distributions' rule): run in float64 it would shut its gradients at 2.2e-16
    # where the definition the kernels implement (include/ddrl.h) says 2^-23.  The float32 eps whatever the dtype; inside the interval --
    # every cell but the saturated one -- these are the same numbers
    logits = torch.log(torch.clamp(p_hat, O.EPS, 1.0 - O.EPS))
    v = v.squeeze(-1)
    log_p = O.categorical_log_prob(logits, actions)
    ratio = torch.exp(log_p - old_logps)
    m = torch.min(ratio * advs, torch.clamp(ratio, 1.0 - O.PPO_CLIP, 1.0 + O.PPO_CLIP) * advs)
    actor_loss = -torch.mean(torch.where(advs > 0, m, torch.max(m, O.DUEL_PPO_CLIP * advs)))
    v_el = element(rets - v, smooth_l1)
    if value_clip > 0:
        v_c = old_values + torch.clamp(v - old_values, -value_clip, value_clip)
        v_el = torch.max(v_el, element(rets - v_c, smooth_l1))
    return actor_loss, v_el.mean(), torch.mean(O.categorical_entropy(p_hat, logits))


def atari_old_values(cell, weights, frames, rets):
    """old_values fp32 [n] of a cell of the context test: the float64 oracle's value minus d, d / VALUE_CLIP cycling through D_OVER_C
    (d_index), and the margins that keep every clip decision the same in fp32 -- | |d| - c | > 1e-3 and, where clipped, the two elements
    more than 1e-4 apart -- asserted here (tests/test_loss_options_cpu.py runs this for every cell)."""
    from oracle import ddrl_oracle as O
    import parity_util as P
    net = (O.OracleSharedPPO if cell.shared else O.OraclePPO)(n_actions=cell.A, num_inputs=cell.C)
    net.load_weights(weights)
    net.double()
    threads = torch.get_num_threads()
    torch.set_num_threads(P.oracle_threads())
    try:
        with torch.no_grad():
            v = net(O.frames_to_f32(frames).double())[3][:, 0]
    finally:
        torch.set_num_threads(threads)
    n = cell.n
    d_over_c = torch.tensor([D_OVER_C[d_index(i)] for i in range(n)], dtype=torch.float64)
    old = (v - d_over_c * VALUE_CLIP).float()
    d = v - old.double()
    ret = torch.from_numpy(np.asarray(rets)).double()
    v_c = old.double() + torch.clamp(d, -VALUE_CLIP, VALUE_CLIP)
    l_u, l_c = element(ret - v, bool(cell.smooth_l1)), element(ret - v_c, bool(cell.smooth_l1))
    assert float((d.abs() - VALUE_CLIP).abs().min()) > 1e-3
    clipped = d.abs() > VALUE_CLIP
    assert bool(clipped.any()) and bool((~clipped).any())
    assert float((l_u - l_c).abs()[clipped].min()) > 1e-4, float((l_u - l_c).abs()[clipped].min())
    if n >= 33:     # both sides of the maximum among the clipped samples (a handful of samples holds what it holds)
        assert bool((l_u > l_c)[clipped].any()) and bool((l_u < l_c)[clipped].any())
    return old.numpy()


def atari_oracle64(hp, shared, weights, frames, actions, old_logps, advs, rets, old_values, smooth_l1, options, **net_args):
    """The float64 oracle's backward under the kernel's leaky-ReLU decisions (test_gpu_parity._adopt_kernel_decisions) with the options
    applied to the oracle nets' outputs; call hp.ppo_iter on the same batch first.  Returns (net with gradients, [actor, v, entropy])."""
    from oracle import ddrl_oracle as O
    import parity_util as P
    from test_gpu_parity import _adopt_kernel_decisions, _release_decisions
    value_clip, split = options
    cls = O.OracleSharedPPO if shared else O.OraclePPO
    n = frames.shape[0]
    x = O.frames_to_f32(frames)
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    threads = torch.get_num_threads()
    torch.set_num_threads(P.oracle_threads())
    try:
        net32 = cls(**net_args)
        net32.load_weights(weights)
        _adopt_kernel_decisions(hp, net32, n, x)
        net = cls(**net_args)
        net.load_weights(weights)
        net.double()
        for a, b in zip([m for m in net.modules() if isinstance(m, O.Encoder)], [m for m in net32.modules() if isinstance(m, O.Encoder)]):
            a.forced, a.tap = b.forced, {}
        net.zero_grad()
        al, vl, ent = atari_losses(net, x.double(), t(actions), t(old_logps), t(advs), t(rets), t(old_values), smooth_l1, value_clip)
        if shared:
            (al + O.V_LOSS_THETA * vl - O.ENT_LOSS_THETA * ent).backward()
        else:
            ((al - O.ENT_LOSS_THETA * ent) if split else al).backward(retain_graph=True)
            vl.backward()
        _release_decisions(net32)
    finally:
        torch.set_num_threads(threads)
    return net, [al.item(), vl.item(), ent.item()]


# ---- PPO.learn against the C API driven by hand -----------------------------------------------------------------------------------------------
LOSS_KEYS = ("PpoTotalLoss", "ActorLoss", "VLoss", "EntLoss")
N_ENVS, HORIZON, CH, ACTIONS = 8, 8, 4, 6


def make_net(seed=3, max_batch=N_ENVS * HORIZON, iters=1, **options):
    """The Atari PPO net (C = 4, A = 6) through create_net with config_nn options set by name, recipe weights loaded."""
    import types
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.utils.recipe import make_weights
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": CH, "discrete_action": True,
           "discrete_actions": list(range(ACTIONS)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg_nn = ConfigNN(env)
    cfg_nn.TRAINING_ITER_TIME = iters
    for k, v in options.items():
        setattr(cfg_nn, k, v)
    net = create_net({"config": BaseConfig(types.SimpleNamespace(task="loss_options", ip="127.0.0.1"), env), "config_nn": cfg_nn,
                      "config_env": env}, max_batch=max_batch)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_weights(seed, num_inputs=CH, n_actions=ACTIONS).items()})
    return net


def rollout(kind, net):
    """One finished 8-env x 8-step rollout of `kind` ("DeviceRollout" / "PlaneRollout") acted by `net`: random frames, rewards in
    {-1, 0, 1}, a done in one step of five."""
    from ddrl4nav_amd import agent
    rng = np.random.default_rng(808)
    N, T = N_ENVS, HORIZON
    frames = rng.integers(0, 256, size=(T + 1, N, 84, 84), dtype=np.uint8)
    rewards = rng.choice(np.array([-1, 0, 1], np.float32), size=(T + 1, N)).astype(np.float32)
    dones = (rng.random((T + 1, N)) < 0.2).astype(np.uint8)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ro = getattr(agent, kind)(net, N, horizon=T, channels=CH, seed=11)
    for t in range(T + 1):
        ro.put_new_frames(t, d(frames[t]), reset=True if t == 0 else None)
        ro.act(t)
        ro.record(t, d(rewards[t]), d(dones[t]))
    ro.finish()
    torch.cuda.synchronize()
    return ro


def run_learn(net, exp):
    out = []
    for ld, update_time, last in net.learn(exp):
        assert last is True
        out.append(({k: ld[k] for k in LOSS_KEYS}, update_time))
    return out


def hand_loop(net, frames, columns, old_values, steps, options, rates=None):
    """Drive `net` (built WITHOUT the knobs) through the C API by hand: per index tensor of `steps` one ddrl_ppo_iter_opt on samples cut
    with torch indexing (ddrl_ppo_iter when both options are off), all-reduce, Adam step; rates: per step the four numbers handed to
    ddrl_set_rates first, or None.  Returns [(loss dict, update_time)]."""
    from ctypes import byref
    from ddrl4nav_amd import _lib, ops
    from ddrl4nav_amd.ops import _p, _st
    hp = net.hot_path
    out = []
    for i, sel in enumerate(steps):
        sel = sel.cuda()
        cut = [c[sel].contiguous() for c in columns]
        fr = frames[sel].contiguous()
        if rates is not None:
            _lib.check(hp.lib.ddrl_set_rates(hp.ctx, *rates[i]))
        if tuple(options) == ops.NO_LOSS_OPTIONS:
            hp.ppo_iter(fr, *cut)
        else:
            vo = old_values[sel].contiguous() if options[0] > 0 else None
            batch = _lib.PpoBatch(_p(fr), 0, _p(None), _p(cut[0]), _p(cut[1]), _p(cut[2]), _p(cut[3]), _p(vo))
            opt = _lib.LossOptions(float(options[0]), 1 if options[1] else 0)
            _lib.check(hp.lib.ddrl_ppo_iter_opt(hp.ctx, byref(batch), byref(opt), len(sel), len(sel), _st()))
        hp.allreduce_grads()
        hp.clip_adam_step()
        net.update_time += 1
        s = hp.stats()
        out.append(({k: s[k] for k in LOSS_KEYS}, net.update_time))
    return out
