"""What tests/test_minibatch_*.py and tests/minibatch_worker.py share: float64 references of the advantage normalisation, the nets of
the learn tests and the hand-composed minibatch loop -- the parent path's API only (hot_path.ppo_iter / allreduce_grads /
clip_adam_step / stats) on minibatches cut with torch indexing from minibatch.epoch_order / split."""
import types

import numpy as np
import torch

import config_cross as X

U = 2.0 ** -24          # unit roundoff of fp32
LOSS_KEYS = ("PpoTotalLoss", "ActorLoss", "VLoss", "EntLoss")
LOSS_TOL = dict(rtol=2e-5, atol=2e-6)       # the project's loss tolerance (tests/test_config_cross_gpu.py)
C, A = 4, 6


# ---- float64 --------------------------------------------------------------------------------------------------------------------------
def moments64(x):
    x = np.asarray(x, np.float64)
    return float(x.size), float(x.sum()), float((x * x).sum())


def normalized64(a, eps, pool=None):
    """(r, bound): r = (a - mean64) / (std64 + eps) in float64 with the moments of `pool` (default: a itself), ddof = 1 (std 0 for
    one sample), and what four fp32 roundings may move the kernel's result by: the mean and the reciprocal rounded to fp32, the
    subtraction, the multiplication --  4u|r| + 2u|mean64| / (std64 + eps) + 1e-12."""
    a = np.asarray(a, np.float64)
    pool = a if pool is None else np.asarray(pool, np.float64)
    mean = pool.mean()
    std = pool.std(ddof=1) if pool.size >= 2 else 0.0
    r = (a - mean) / (std + eps)
    return r, 4 * U * np.abs(r) + 2 * U * abs(mean) / (std + eps) + 1e-12


# ---- the learn tests ------------------------------------------------------------------------------------------------------------------
def cell(B, shared=0, max_batch=None):
    return X.Cell(C, A, shared, 0, B, B if max_batch is None else max_batch)


def batch_of(cl):
    frames, acts, old, adv, ret, w = X.cell_inputs(cl)
    return {"frames": frames, "actions": acts, "old_logps": old, "advs": adv, "rets": ret}, w


def make_net(weights, max_batch, shared=False, iters=1, **options):
    """The Atari PPO net (C = 4, A = 6) through create_net with config_nn options set by name, recipe weights loaded."""
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.runner import create_net
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": C, "discrete_action": True,
           "discrete_actions": list(range(A)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg_nn = ConfigNN(env)
    cfg_nn.TRAINING_ITER_TIME = iters
    cfg_nn.SHARE_CNN_NET = bool(shared)
    for k, v in options.items():
        setattr(cfg_nn, k, v)
    net = create_net({"config": BaseConfig(types.SimpleNamespace(task="minibatch", ip="127.0.0.1"), env), "config_nn": cfg_nn,
                      "config_env": env}, max_batch=max_batch)
    net.load_state_dict({k: torch.from_numpy(np.array(v, copy=True)) for k, v in weights.items()})
    return net


def experience(batch, lo=0, hi=None):
    from ddrl4nav_amd.data import Experience
    hi = len(batch["actions"]) if hi is None else hi
    exp = Experience(states=[batch["frames"][lo:hi]], advs=batch["advs"][lo:hi], actions=batch["actions"][lo:hi],
                     old_logps=batch["old_logps"][lo:hi], values=batch["rets"][lo:hi].reshape(1, -1))
    exp.to_tensor(dtype=torch.float32, device="cuda")
    return exp


def state_of(net):
    hp = net.hot_path
    return {"params": hp.params.cpu().numpy().copy(), "m": hp.adam_m.cpu().numpy().copy(), "v": hp.adam_v.cpu().numpy().copy(),
            "step": hp.step, "update_time": net.update_time}


def run_learn(net, batch, lo=0, hi=None):
    """[(loss dict without PpoBackUpTime, update_time)] of one net.learn call."""
    out = []
    for ld, update_time, last in net.learn(experience(batch, lo, hi)):
        assert last is True and "PpoBackUpTime" in ld
        out.append(({k: v for k, v in ld.items() if k != "PpoBackUpTime"}, update_time))
    return out


def step_indices(seed, learn_call, epochs, B, K, shuffle):
    """[int64 index tensor per step] of a learn call: epoch_order (or storage order) cut by split."""
    from ddrl4nav_amd.nn import minibatch as M
    out = []
    for e in range(epochs):
        order = M.epoch_order(seed, learn_call, e, B).long() if shuffle else torch.arange(B)
        out += [order[lo:hi] for lo, hi in M.split(B, K)]
    return out


def hand_loop(net, batch, steps, mode=None, eps=1e-8, max_steps=None, b_globals=None):
    """Drive `net` (built WITHOUT the knobs) by hand over the index tensors `steps`; the advantages normalised with the operators the
    kernel tests check (mode "batch": once over the whole batch; "minibatch": per step).  Returns [(loss dict, update_time)]."""
    from ddrl4nav_amd import ops
    hp = net.hot_path
    d = lambda k: torch.from_numpy(np.ascontiguousarray(batch[k])).cuda()
    frames, acts, old, advs, rets = d("frames"), d("actions"), d("old_logps"), d("advs"), d("rets")
    if mode == "batch":
        advs = ops.normalize(advs, ops.moments_affine(ops.moments(advs), eps))
    out = []
    for i, sel in enumerate(steps[:max_steps]):
        sel = sel.cuda()
        ad = advs[sel].contiguous()
        if mode == "minibatch":
            ad = ops.normalize(ad, ops.moments_affine(ops.moments(ad), eps))
        hp.ppo_iter(frames[sel].contiguous(), acts[sel].contiguous(), old[sel].contiguous(), ad, rets[sel].contiguous(),
                    b_global=None if b_globals is None else b_globals[i])
        hp.allreduce_grads()
        hp.clip_adam_step()
        net.update_time += 1
        s = hp.stats()
        out.append(({k: s[k] for k in LOSS_KEYS}, net.update_time))
    return out


def oracle_losses64(weights, batch, sel, advs64, shared=False):
    """[actor_loss, v_loss, entropy] of the float64 oracle on the samples `sel` with the float64 advantages given."""
    from oracle import ddrl_oracle as O
    import parity_util as P
    net = (O.OracleSharedPPO if shared else O.OraclePPO)(n_actions=A, num_inputs=C)
    net.load_weights(weights)
    net.double()
    sel = np.asarray(sel)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    threads = torch.get_num_threads()
    torch.set_num_threads(P.oracle_threads())
    try:
        with torch.no_grad():
            _, al, vl, ent = O.ppo_losses(net, O.frames_to_f32(batch["frames"][sel]).double(), t(batch["actions"][sel]),
                                          t(batch["old_logps"][sel]), t(advs64), t(batch["rets"][sel]), False)
    finally:
        torch.set_num_threads(threads)
    return [al.item(), vl.item(), ent.item()]
