"""The host side of the PPO update diagnostics (ops.diag_dict, the rank combination, the option guards, the trainer's logging) and the
promises the GPU tests lean on (tests/test_ppo_diag_gpu.py): for every case of its operator grid the float64 reference and its own
fp32 run count the same clipped samples.  No GPU."""
import math
import types

import numpy as np
import pytest
import torch

import heads_ref as H
import ppo_diag_ref as R
from ddrl4nav_amd import ops


def _sums(x, ret, v, clip):
    r = torch.exp(x)
    e = ret - v
    return [float(len(x)), float((torch.expm1(x) - x).sum()), float(R.clipped_count(r, clip)), float(ret.sum()), float((ret * ret).sum()),
            float(e.sum()), float((e * e).sum()), float(r.max())]


def test_diag_dict_against_direct_float64():
    g = torch.Generator().manual_seed(5)
    for n in (1, 7, 1000):
        x = torch.randn(n, generator=g, dtype=torch.float64) * 0.3
        ret = torch.randn(n, generator=g, dtype=torch.float64) * 2.0 + 1.0
        v = ret + torch.randn(n, generator=g, dtype=torch.float64) * 0.5
        got = ops.diag_dict(_sums(x, ret, v, 0.2))
        want = R.direct_diag(x, ret, v, 0.2)
        assert set(got) == set(ops.DIAG_KEYS) == set(want)
        for k in ("ApproxKL", "ClipFraction", "RatioMax"):
            assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-15), (n, k)
        if n == 1:
            assert math.isnan(got["ExplainedVariance"]) and math.isnan(want["ExplainedVariance"])
        else:
            assert got["ExplainedVariance"] == pytest.approx(want["ExplainedVariance"], rel=1e-9), n
        assert got["ApproxKL"] >= 0.0


def test_diag_dict_accepts_tensors_and_arrays():
    s = [4.0, 0.02, 1.0, 2.0, 3.0, 0.5, 0.75, 1.5]
    a = ops.diag_dict(s)
    assert a == ops.diag_dict(np.asarray(s)) == ops.diag_dict(torch.tensor(s, dtype=torch.float64))
    assert a["ApproxKL"] == 0.005 and a["ClipFraction"] == 0.25 and a["RatioMax"] == 1.5


def test_explained_variance_is_nan_on_constant_returns():
    n = 64
    ret = torch.full((n,), 3.0, dtype=torch.float64)
    v = torch.randn(n, dtype=torch.float64)
    d = ops.diag_dict(_sums(torch.zeros(n, dtype=torch.float64), ret, v, 0.2))
    assert math.isnan(d["ExplainedVariance"])
    assert d["ApproxKL"] == 0.0 and d["ClipFraction"] == 0.0 and d["RatioMax"] == 1.0


def test_rank_combination_sums_the_parts_and_takes_the_largest_ratio():
    g = torch.Generator().manual_seed(9)
    n = 64
    x = torch.randn(n, generator=g, dtype=torch.float64) * 0.3
    ret = torch.randn(n, generator=g, dtype=torch.float64)
    v = torch.randn(n, generator=g, dtype=torch.float64)
    whole = _sums(x, ret, v, 0.2)
    parts = [_sums(x[lo:hi], ret[lo:hi], v[lo:hi], 0.2) for lo, hi in ((0, 40), (40, 64))]
    got = ops.combine_diag_sums(parts)
    for k in range(7):
        assert got[k] == pytest.approx(whole[k], rel=1e-12, abs=1e-12)
    assert got[0] == 64.0 and got[2] == whole[2]
    assert got[7] == whole[7] == max(p[7] for p in parts)
    # the fold is in the order given and nothing else: what two ranks compute from the same gathered rows is the same bits
    assert ops.combine_diag_sums([torch.tensor(p, dtype=torch.float64) for p in parts]) == got
    assert ops.combine_diag_sums([parts[0]]) == [float(t) for t in parts[0]]
    from ddrl4nav_amd.dist import allgather_diag_sums
    assert allgather_diag_sums(parts[0]) == [float(t) for t in parts[0]]      # one process: the row itself


def test_option_guards():
    ns = types.SimpleNamespace
    assert ops.diag_options(ns()) == (False, None)
    assert ops.diag_options(ns(PPO_DIAGNOSTICS=True)) == (True, None)
    assert ops.diag_options(ns(TARGET_KL=0.02)) == (True, 0.02)          # a target implies the diagnostics
    assert ops.diag_options(ns(DEFERRED_LOSS_READBACK=True, PPO_DIAGNOSTICS=True)) == (True, None)
    with pytest.raises(ValueError) as e:
        ops.diag_options(ns(TARGET_KL=0.02, DEFERRED_LOSS_READBACK=True))
    assert "TARGET_KL" in str(e.value) and "DEFERRED_LOSS_READBACK" in str(e.value)
    with pytest.raises(ValueError):
        ops.diag_options(ns(TARGET_KL=0.0))
    assert ops.kl_stop({"ApproxKL": 0.031}, 0.02) and not ops.kl_stop({"ApproxKL": 0.03}, 0.02)
    assert not ops.kl_stop({"ApproxKL": 1.0}, None)


def _atari_configs(network_type="ppo", **options):
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": 4, "discrete_action": True,
           "discrete_actions": list(range(6)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg_nn = ConfigNN(env)
    cfg_nn.NETWORK_TYPE = network_type
    for k, v in options.items():
        setattr(cfg_nn, k, v)
    return {"config": BaseConfig(types.SimpleNamespace(task="diag", ip="127.0.0.1"), env), "config_nn": cfg_nn, "config_env": env}


def test_config_contract_does_not_carry_the_options():
    cfg_nn = _atari_configs()["config_nn"]
    assert not hasattr(cfg_nn, "PPO_DIAGNOSTICS") and not hasattr(cfg_nn, "TARGET_KL")


def test_constructors_refuse_what_is_not_built():
    from ddrl4nav_amd.runner import create_net
    # the Atari learner: refused before anything touches a device
    with pytest.raises(ValueError) as e:
        create_net(_atari_configs(TARGET_KL=0.01, DEFERRED_LOSS_READBACK=True), max_batch=8)
    assert "TARGET_KL" in str(e.value) and "DEFERRED_LOSS_READBACK" in str(e.value)
    for opt in (dict(PPO_DIAGNOSTICS=True), dict(TARGET_KL=0.01)):
        with pytest.raises(NotImplementedError) as e:
            create_net(_atari_configs("gail", SHARE_CNN_NET=True, **opt), max_batch=8)
        assert "gail" in str(e.value)


def test_trainer_logs_the_keys_learn_yields_unchanged():
    """server/backward.py hands every key of a yielded loss dict to the logger under its own name."""
    from ddrl4nav_amd.server.backward import BackwardTrainer
    item = {"PpoTotalLoss": 1.0, "ActorLoss": 0.5, "VLoss": 0.25, "EntLoss": 0.125, "PpoBackUpTime": 0.0, "ApproxKL": 0.01,
            "ClipFraction": 0.25, "ExplainedVariance": -0.5, "RatioMax": 1.75}

    class Net:
        device = "cpu"

        def learn(self, data):
            yield dict(item), 1, True

    class Data:
        def to_tensor(self, **kw):
            pass

        def __len__(self):
            return 4

    config = types.SimpleNamespace(TASK_NAME="t", UPDATE_TAG_KEY="u", TRAIN_LOCK_KEY="l", LOG_LOSS_FREQUENCY=1, SAVE_MODELS=False,
                                   SAVE_FREQUENCY=1, SAVE_MODEL_PATH="", LOAD_CHECKPOINT=False)
    config_nn = types.SimpleNamespace(MODEL_TO_REDIS_FREQUENCY=10, MODULE_TENSOR_DTYPE=torch.float32, TRAINING_MIN_BATCH=4)
    seen = {}
    tr = BackwardTrainer(Net(), config, config_nn, log=lambda k, v, step: seen.__setitem__(k, v))
    tr.consume(Data())
    assert seen == item


@pytest.mark.parametrize("cont,A,shared,below", R.GRID, ids=[R.case_id(*g) for g in R.GRID])
def test_float64_and_fp32_references_count_the_same_clipped_samples(cont, A, shared, below):
    """The GPU test asks for the clipped COUNT to match exactly: the recipe keeps every ratio at least 0.1 from 1 +- clip, so a
    log-prob error of fp32 size cannot move a sample across -- checked here on the reference's own fp32 run, for every case."""
    for n in R.NS:
        c = R.make_case(cont, A, n, shared)
        clip = c.hyper["ppo_clip"]
        r64, r32 = R.per_sample(c, torch.float64)[3], R.per_sample(c, torch.float32)[3]
        assert float(((r64 - 1.0).abs() - clip).abs().min()) > 0.05
        assert R.clipped_count(r64, clip) == R.clipped_count(r32.double(), clip)
        lo, hi = np.float32(1.0) - np.float32(clip), np.float32(1.0) + np.float32(clip)     # the kernel's form of the same test
        assert int(((r32 < lo) | (r32 > hi)).sum()) == R.clipped_count(r64, clip)
        if n >= 33:
            assert 0 < R.clipped_count(r64, clip) < n
