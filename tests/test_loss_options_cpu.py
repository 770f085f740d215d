"""The PPO update options where no GPU is needed: the recipe of tests/test_loss_options_gpu.py keeps its promises
over the whole GPU grid, the float32 restatement of the option loss block sits within HALF the bound the GPU test applies to the kernels
(the rule of tests/test_config_cross_cpu.py), the option validators and the GAIL refusals, the header against the binding, the anneal
factor's arithmetic, and PPO.learn's refusal of a batch without the collecting policy's values."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import heads_ref as H
import loss_options_ref as LR

OP_TOL = 2e-5     # tests/test_heads_optim_ops_gpu.py: what every row / tensor of the kernels is held to
CASES = LR.loss_cases()


# ---- the recipe -------------------------------------------------------------------------------------------------------------------------
def test_grid_covers_what_it_says():
    assert len(CASES) == len(set(CASES))
    for cont, sizes in ((0, (6, 8, 18)), (1, (2, 8))):
        mine = [c for c in CASES if c[0] == cont]
        assert {c[1] for c in mine} == set(sizes)
        for A in sizes:
            ns = sorted({c[2] for c in mine if c[1] == A})
            assert ns[:4] == [1, 3, 5, 67] and ns[4] == LR.full_pass(cont, A) + 3 and ns[4] % 4 != 0
        for name in LR.OPTION_SETS:
            sub = [c for c in mine if c[5] == name]
            assert {c[3] for c in sub} == {0, 1} and {c[4] for c in sub} == {0, 1}, (cont, name)
            assert {c[2] for c in sub} >= {1, 3, 5, 67} and max(c[2] for c in sub) > 1000
    # the three kernel classes of the Categorical head take 8, 4 and 4 waves of 4 samples; the Gaussian head 4 waves of one
    assert (LR.full_pass(0, 6), LR.full_pass(0, 8), LR.full_pass(0, 18), LR.full_pass(1, 2)) == (8192, 4096, 4096, 1024)


def test_d_cycle_meets_every_return_distance():
    pairs = {(i % 7, LR.d_index(i)) for i in range(49)}
    assert len(pairs) == 49 and {(i % 7, LR.d_index(i)) for i in range(64)} == pairs


@pytest.mark.parametrize("spec", CASES, ids=LR.case_id)
def test_recipe_keeps_its_margins_and_fp32_stays_inside_half_the_gpu_bound(spec):
    c = LR.case_of(spec)
    LR.check_recipe(c)
    r64, r32 = LR.loss_block(c, torch.float64), LR.loss_block(c, torch.float32)
    # the option did something to the reference (else the GPU test would show nothing): against the plain block of heads_ref
    plain = H.loss_block(c, torch.float64)
    if c.value_clip > 0 and c.n >= 3:
        assert float((r64["losses"][1] - plain["losses"][1]).abs()) > 1e-6
    if c.entropy_split and not c.shared:
        moved = "g_log_std" if c.continuous else "dh_actor"      # a Normal's entropy depends on log_std alone
        assert float((r64[moved] - plain[moved]).abs().max()) > 0
        assert torch.equal(r64["dh_critic"], LR.loss_block(LR.make_case(*spec[:5], (c.value_clip, False), seed=2, B_global=spec[6]),
                                                           torch.float64)["dh_critic"])      # the value side is unchanged
    assert torch.equal(r64["losses"][[0, 2]], plain["losses"][[0, 2]])                      # actor loss and entropy: statistics unchanged
    noise = c.err64.abs() < 1e-3     # rows whose value gradient is rounding noise in float64 itself (check_heads_loss holds them apart)
    for name in ("dh_actor", "dh_critic"):
        if r64[name] is None:
            continue
        scale = r64[name].abs().amax(1)
        live = (scale > 0) & ~(noise if (name == "dh_critic" or c.shared) else torch.zeros_like(noise))
        dead = scale == 0
        assert bool((r32[name][dead] == 0).all()), name          # the same branch decisions in fp32: exact zeros where float64 has them
        if bool(live.any()):
            err = ((r32[name] - r64[name]).abs().amax(1) / scale.clamp_min(1e-300))[live]
            assert float(err.max()) <= OP_TOL / 2, (name, float(err.max()))
    for k in ("g_actor_w", "g_critic_w", "g_actor_b", "g_critic_b") + (("g_log_std",) if c.continuous else ()):
        scale = float(r64[k].abs().max())
        if scale == 0:
            assert bool((r32[k] == 0).all()), k
            continue
        assert float((r32[k] - r64[k]).abs().max()) <= OP_TOL / 2 * scale + 0.5e-7, k
    assert float((r32["losses"] - r64["losses"]).abs().max()) <= OP_TOL / 2 * float(r64["losses"].abs().max()) + 0.5e-7


def test_context_cells_keep_their_clip_margins():
    import config_cross as X
    from test_loss_options_gpu import CELLS
    assert {(c.A <= 6, 6 < c.A <= 8, c.A > 8) for c, _ in CELLS} == {(True, False, False), (False, True, False), (False, False, True)}
    assert {c.shared for c, _ in CELLS} == {0, 1} and {c.smooth_l1 for c, _ in CELLS} == {0, 1}
    assert {n for _, n in CELLS} == set(LR.OPTION_SETS)
    for cell, _ in CELLS:
        frames, _, _, _, ret, w = X.cell_inputs(cell)
        old = LR.atari_old_values(cell, w, frames, ret)
        assert old.shape == (cell.n,) and old.dtype == np.float32


def test_reference_gradient_conventions():
    """The float64 reference itself on a hand-made case: inside the clip the two elements tie and the gradient is the unclipped one;
    clipped with the clipped element larger the value gradient is exactly zero; clipped with the unclipped one larger it is as without."""
    c = LR.make_case(0, 6, 67, 0, 0, LR.OPTION_SETS["clip"], seed=2)
    r, plain = LR.loss_block(c, torch.float64), H.loss_block(c, torch.float64)
    out = LR.clip_outcomes(c)
    rows, prow = r["dh_critic"].abs().amax(1), plain["dh_critic"].abs().amax(1)
    for i, o in enumerate(out):
        if o == "clipped_clipped_larger":
            assert float(rows[i]) == 0.0
        elif o == "clipped_unclipped_larger":
            assert torch.equal(r["dh_critic"][i], plain["dh_critic"][i])
        else:
            assert abs(float(rows[i]) - float(prow[i])) <= 1e-6 * max(float(prow[i]), 1e-12) + 1e-12


# ---- validators -------------------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    return types.SimpleNamespace(**kw)


def test_option_validators():
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.nn import minibatch as M
    assert M.value_clip_option(_cfg()) is None and M.value_clip_option(_cfg(VALUE_CLIP=None)) is None
    assert M.value_clip_option(_cfg(VALUE_CLIP=False)) is None and M.value_clip_option(_cfg(VALUE_CLIP=0.2)) == 0.2
    assert M.value_clip_option(_cfg(VALUE_CLIP=1)) == 1.0
    for bad in (0, 0.0, -0.1, float("nan"), float("inf"), True, "0.2"):
        with pytest.raises(ValueError, match="VALUE_CLIP"):
            M.value_clip_option(_cfg(VALUE_CLIP=bad))
    assert M.entropy_split_option(_cfg()) is False and M.entropy_split_option(_cfg(ENTROPY_BONUS_SPLIT=True)) is True
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="ENTROPY_BONUS_SPLIT"):
            M.entropy_split_option(_cfg(ENTROPY_BONUS_SPLIT=bad))
    assert M.loss_options(_cfg()) == ops.NO_LOSS_OPTIONS == (0.0, False)
    assert M.loss_options(_cfg(VALUE_CLIP=0.3, ENTROPY_BONUS_SPLIT=True)) == (0.3, True)
    assert M.anneal_options(_cfg()) is None and M.anneal_options(_cfg(LR_ANNEAL_UPDATES=None)) is None
    assert M.anneal_options(_cfg(LR_ANNEAL_UPDATES=4)) == (4, 0.0, False)
    assert M.anneal_options(_cfg(LR_ANNEAL_UPDATES=10, LR_ANNEAL_FLOOR=0.25, CLIP_ANNEAL=True)) == (10, 0.25, True)
    for bad in (0, -1, 2.5, True, "4"):
        with pytest.raises(ValueError, match="LR_ANNEAL_UPDATES"):
            M.anneal_options(_cfg(LR_ANNEAL_UPDATES=bad))
    for bad in (-0.1, 1.5, float("nan"), None, True):
        with pytest.raises(ValueError, match="LR_ANNEAL_FLOOR"):
            M.anneal_options(_cfg(LR_ANNEAL_UPDATES=4, LR_ANNEAL_FLOOR=bad))
    with pytest.raises(ValueError, match="CLIP_ANNEAL"):
        M.anneal_options(_cfg(LR_ANNEAL_UPDATES=4, CLIP_ANNEAL=1))
    for orphan in (dict(CLIP_ANNEAL=True), dict(LR_ANNEAL_FLOOR=0.5)):
        with pytest.raises(ValueError, match="LR_ANNEAL_UPDATES"):
            M.anneal_options(_cfg(**orphan))


ENV = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": 4, "discrete_action": True,
       "discrete_actions": list(range(6)), "agent_num_per_env": 1, "batch_num_per_env": 8}


def _config_nn(**options):
    from ddrl4nav_amd.config import ConfigNN
    cfg_nn = ConfigNN(ENV)
    for k, v in options.items():
        setattr(cfg_nn, k, v)
    return cfg_nn


def test_gail_refuses_the_loss_options():
    from ddrl4nav_amd.nn import minibatch as M
    from ddrl4nav_amd.nn.gail import GAIL
    M.refuse_loss_options(_cfg(), "x")
    M.refuse_loss_options(_cfg(LR_ANNEAL_UPDATES=4), "x")         # the schedules are not refused
    for opts in (dict(VALUE_CLIP=0.2), dict(ENTROPY_BONUS_SPLIT=True)):
        with pytest.raises(ValueError, match="VALUE_CLIP / ENTROPY_BONUS_SPLIT"):
            M.refuse_loss_options(_cfg(**opts), "NETWORK_TYPE='gail'")
        disc = types.SimpleNamespace(config=None, config_nn=_config_nn(**opts), device="cpu")
        with pytest.raises(ValueError, match="VALUE_CLIP / ENTROPY_BONUS_SPLIT"):
            GAIL(generator=None, discriminator=disc, gail_critic=None)
    # a generator built with the options is refused as well, whatever the discriminator's configuration says
    disc = types.SimpleNamespace(config=None, config_nn=_config_nn(), device="cpu")
    with pytest.raises(ValueError, match="generator"):
        GAIL(generator=types.SimpleNamespace(loss_options=(0.2, False)), discriminator=disc, gail_critic=None)


def test_create_net_refuses_the_loss_options_for_gail():
    from ddrl4nav_amd.config import BaseConfig
    from ddrl4nav_amd.runner import create_net
    for opts in (dict(VALUE_CLIP=0.2), dict(ENTROPY_BONUS_SPLIT=True)):
        cfg_nn = _config_nn(NETWORK_TYPE="gail", SHARE_CNN_NET=True, **opts)
        with pytest.raises(ValueError, match="VALUE_CLIP / ENTROPY_BONUS_SPLIT"):
            create_net({"config": BaseConfig(types.SimpleNamespace(task="t", ip="127.0.0.1"), ENV), "config_nn": cfg_nn, "config_env": ENV})


# ---- the header against the binding --------------------------------------------------------------------------------------------------------
NEW_NAMES = ("ddrl_ppo_iter_opt", "ddrl_op_heads_loss_opt", "ddrl_set_rates", "ddrl_op_gather_f32", "ddrl_loss_options")


def test_header_and_binding_agree_on_the_new_names():
    from ddrl4nav_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ddrl.h")).read(), flags=re.S)
    assert "#define DDRL_ABI_VERSION 3" in src and _lib.ABI_VERSION == 3
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_NAMES[:4]:
        m = re.search(r"int32_t %s\((.*?)\);" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    m = re.search(r"typedef struct ddrl_loss_options \{(.*?)\} ddrl_loss_options;", src, flags=re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "float value_clip; int32_t entropy_split; int32_t reserved[2];"
    assert [f[0] for f in _lib.LossOptions._fields_] == ["value_clip", "entropy_split", "reserved"] and ctypes.sizeof(_lib.LossOptions) == 16
    m = re.search(r"typedef struct ddrl_ppo_batch \{(.*?)\} ddrl_ppo_batch;", src, flags=re.S)
    fields = re.findall(r"\*?\s*\**(\w+)\s*[,;]", m.group(1))
    assert fields == [f[0] for f in _lib.PpoBatch._fields_] == ["frames_or_planes", "n_planes", "tab", "actions", "old_logps", "advs",
                                                                 "rets", "old_values"]
    assert ctypes.sizeof(_lib.PpoBatch) == 64
    # ddrl_config is what it was: the options did not go into it
    assert [f[0] for f in _lib.Config._fields_][-1] == "smooth_l1_loss" and ctypes.sizeof(_lib.Config) == 68


def test_argument_checks_answer_without_a_gpu():
    """Every check of the new entry points that comes before the context or HIP is touched (a NULL context is refused last)."""
    from ctypes import byref
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    for bad in ((-1e-5, 1e-3, 2e-4, 0.2), (5e-5, nan, 2e-4, 0.2), (5e-5, 1e-3, inf, 0.2), (5e-5, 1e-3, 2e-4, -0.2), (5e-5, 1e-3, 2e-4, nan)):
        assert lib.ddrl_set_rates(None, *bad) == -1
    assert lib.ddrl_set_rates(None, 5e-5, 1e-3, 2e-4, 0.2) == -1           # no context
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    batch = _lib.PpoBatch(p, 0, None, p, p, p, p, None)
    for opt in (_lib.LossOptions(-0.1, 0), _lib.LossOptions(nan, 0), _lib.LossOptions(inf, 0), _lib.LossOptions(0.2, 0),      # clip without old_values
                _lib.LossOptions(0.0, 1, (ctypes.c_int32 * 2)(0, 1)), _lib.LossOptions(0.0, 1, (ctypes.c_int32 * 2)(1, 0))):
        assert lib.ddrl_ppo_iter_opt(None, byref(batch), byref(opt), 1, 1, None) == -1
    batch.old_values = p.value + 2                                          # misaligned
    assert lib.ddrl_ppo_iter_opt(None, byref(batch), byref(_lib.LossOptions(0.2, 0)), 1, 1, None) == -1
    assert lib.ddrl_ppo_iter_opt(None, None, byref(_lib.LossOptions(0.0, 1)), 1, 1, None) == -1
    assert lib.ddrl_ppo_iter_opt(None, byref(batch), None, 1, 1, None) == -1
    tabbed = _lib.PpoBatch(p.value + 4, 1, p, p, p, p, p, None)             # table form: planes 16-byte aligned, n_planes >= 1
    assert lib.ddrl_ppo_iter_opt(None, byref(tabbed), byref(_lib.LossOptions(0.0, 1)), 1, 1, None) == -1
    # gather_f32: NULLs, sizes, alignment, overlap -- before any launch
    src, dst = p.value, p.value + 16
    assert lib.ddrl_op_gather_f32(None, 4, None, 0, 2, dst, None) == -1 and lib.ddrl_op_gather_f32(src, 4, None, 0, 2, None, None) == -1
    assert lib.ddrl_op_gather_f32(src, 0, None, 0, 2, dst, None) == -1 and lib.ddrl_op_gather_f32(src, 4, None, 0, 0, dst, None) == -1
    assert lib.ddrl_op_gather_f32(src + 2, 4, None, 0, 2, dst, None) == -1 and lib.ddrl_op_gather_f32(src, 4, src + 1, 0, 2, dst, None) == -1
    assert lib.ddrl_op_gather_f32(src, 6, None, 0, 2, dst, None) == -1      # dst inside src
    assert lib.ddrl_op_gather_f32(src, 2, dst, 0, 2, dst, None) == -1       # dst is idx
    # heads_loss_opt: the options' own checks come first
    for opt in (_lib.LossOptions(-1.0, 0), _lib.LossOptions(nan, 0), _lib.LossOptions(0.2, 0)):
        assert lib.ddrl_op_heads_loss_opt(None, None, None, None, None, 1, None, None, None, None, byref(opt), None, 1, None, None, None,
                                          None, None) == -1


# ---- annealing ------------------------------------------------------------------------------------------------------------------------------
def test_anneal_factor_arithmetic():
    from ddrl4nav_amd.nn import minibatch as M
    N = 4
    assert [M.anneal_factor(u, N) for u in (0, N - 1, N, N + 3)] == [1.0, 0.25, 0.0, 0.0]
    assert [M.anneal_factor(u, N, 0.3) for u in (0, 2, N - 1, N, 9)] == [1.0, 0.5, 0.3, 0.3, 0.3]
    assert M.anneal_factor(1, 3) == 1.0 - 1.0 / 3.0 and M.anneal_factor(0, 1) == 1.0 and M.anneal_factor(1, 1, 1.0) == 1.0
    base = (5e-5, 1e-3, 2e-4, 0.2)
    for u in (0, 1, 3, 4, 7):
        for floor, clip in ((0.0, False), (0.1, True)):
            got = M.annealed_rates(base, u, 7, floor, clip)
            s = max(floor, 1.0 - u / 7.0)
            assert got == (5e-5 * s, 1e-3 * s, 2e-4 * s, 0.2 * s if clip else 0.2)                  # formed in double
            assert [float(np.float32(x)) for x in got] == LR.annealed_rates32(base, u, 7, floor, clip)   # rounded once
    # u = 0 leaves the fp32 numbers of the configuration as they are
    assert LR.annealed_rates32(base, 0, 5) == [float(np.float32(x)) for x in base]


# ---- PPO.learn without the collecting policy's values -----------------------------------------------------------------------------------------
def test_learn_raises_without_row_1():
    """The check comes before anything is launched: a stand-in for the net shows it on a host without a GPU."""
    from ddrl4nav_amd.data import Experience
    from ddrl4nav_amd.nn.minibatch import DEFAULTS
    from ddrl4nav_amd.nn.ppo import PPO
    B = 5
    fake = types.SimpleNamespace(device=torch.device("cpu"), loss_options=(0.2, False), wants_old_values=True, minibatch=DEFAULTS,
                                 training_iter_time=1)
    frames = torch.zeros((B, 4, 84, 84), dtype=torch.uint8)
    col = torch.zeros(B)
    exp = Experience(states=[frames], advs=col, actions=col, old_logps=col, values=torch.zeros(1, B))
    with pytest.raises(ValueError, match="VALUE_CLIP"):
        next(PPO.learn(fake, exp))
