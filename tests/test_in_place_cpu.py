"""Host side of learning in place (csrc/ftable.hip's and ddrl_ppo_iter_indexed's argument checks; the header; the FRAMES_IN_PLACE knob
and its guards) and the numpy model of the frame tables the GPU tests lean on (tests/frame_table_ref.py) against the literal deque
model of FrameStackWrapper.  No GPU: every refusal below is decided before the first HIP call."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import frame_table_ref as F
import plane_pool_ref as R
from test_frame_stack_cpu import episode      # the literal deque model of FrameStackWrapper (DequeStack) run over an episode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddrl_ppo_iter_indexed", "ddrl_op_frame_table_planes", "ddrl_op_frame_table_stacks")
INVALID, UNSUPPORTED = -1, -2


# ---- the numpy model against the deque ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_table_model_names_the_deque_models_frames(C):
    """40 steps of 5 envs with random resets: the planes the table names are the deque's observation at every step, the padding entries
    repeat the last channel, and out-of-range samples name what the clamped sample names."""
    n, steps = 5, 40
    stacks, newest, dones = episode(np.random.default_rng(400 + C), n, C, steps)
    assert dones.any() and not dones.all()
    H = C - 1
    planes = np.concatenate([np.full((H, n, 84, 84), 0xEE, np.uint8), newest])
    age = np.zeros((steps + 1, n), np.uint8)
    age[0] = R.next_age(None, np.ones(n, np.uint8), C)
    for t in range(steps):
        age[t + 1] = R.next_age(age[t], dones[t], C)
    B = (steps + 1) * n
    tab = F.table_planes(age, C, H, n, np.arange(B))
    assert tab.shape == (B, 4) and tab.dtype == np.int32 and tab.min() >= 0 and tab.max() < planes.shape[0] * n
    assert np.array_equal(F.frames_of(planes, tab, C).reshape(stacks.shape), stacks)
    assert (tab[:, C - 1:] == tab[:, C - 1:C]).all()
    assert np.array_equal(F.frames_of(planes, tab, C), R.reconstruct(planes, age, C, np.arange(B)))
    wild = np.array([-1, B, 2 ** 31 - 1, -2 ** 31, 7, 7])
    assert np.array_equal(F.table_planes(age, C, H, n, wild), tab[[0, B - 1, B - 1, 0, 7, 7]])


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_stacked_table_model(C):
    frames = np.random.default_rng(C).integers(0, 256, size=(7, C, 84, 84), dtype=np.uint8)
    idx = np.array([3, 3, 0, 6, -1, 7, 2 ** 31 - 1, -2 ** 31])
    tab = F.table_stacks(7, C, idx)
    assert tab[:, :C].tolist() == [[b * C + c for c in range(C)] for b in (3, 3, 0, 6, 0, 6, 6, 0)]
    assert (tab[:, C - 1:] == tab[:, C - 1:C]).all()
    assert np.array_equal(F.frames_of(frames, tab, C), frames[[3, 3, 0, 6, 0, 6, 6, 0]])
    assert F.clamp_table(np.array([[-1, 0, 7 * C, 7 * C - 1]]), 7 * C).tolist() == [[0, 0, 7 * C - 1, 7 * C - 1]]


# ---- header, binding, library ----------------------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_binds():
    from ddrl4nav_amd import _lib, ops
    from ddrl4nav_amd.data import FramePlanes
    from ddrl4nav_amd.engine import HotPath
    text = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    for name in NEW:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [11, 19, 16]
    assert re.search(r"#define\s+DDRL_ABI_VERSION\s+3\b", text) and _lib.ABI_VERSION == 3      # additive
    assert "CLAMPED" in text                                   # the one difference from the gathers is stated
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW) and lib.ddrl_abi_version() == 3
    assert callable(ops.frame_table_planes) and callable(ops.frame_table_stacks)
    assert callable(HotPath.ppo_iter_indexed) and callable(FramePlanes.table)


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
a, M = 0x100000, 0x100000
COLS = dict(ac=a + 2 * M, ol=a + 3 * M, ad=a + 4 * M, re=a + 5 * M, acd=a + 6 * M, old=a + 7 * M, add=a + 8 * M, red=a + 9 * M)
AGE, IDX, AF, TAB = a + 11 * M, a + M, a + 10 * M, a + 24 * M
NO_COLS = dict(ac=None, acd=None, ol=None, old=None, ad=None, add=None, re=None, red=None, af=None)
# what both builders refuse alike; `samples` entries in every source column, n = 5 table rows of 16 bytes
def shared_refusals(samples):
    return (dict(tab=None), dict(n=0), dict(n=-1), dict(tab=TAB + 2), dict(idx=IDX + 2), dict(af=AF + 1),
            dict(idx=None, first=2 ** 63 - 3),                                  # first + n past int64
            dict(ac=None), dict(acd=None), dict(ol=None), dict(old=None), dict(ad=None), dict(add=None), dict(re=None), dict(red=None),
            dict(ac=a + 2 * M + 2), dict(red=a + 9 * M + 1),
            dict(ad=None, add=None),                                              # an affine without the advantage column
            dict(tab=IDX + 16), dict(tab=IDX - 5 * 16 + 4), dict(tab=AF + 4),     # the table on the indices, on the affine pair
            dict(tab=a + 4 * M + 4 * samples - 4), dict(acd=a + 2 * M + 4), dict(red=a + 5 * M),   # a destination on a source column
            dict(add=IDX + 16), dict(add=AF + 4),
            dict(acd=TAB + 16), dict(red=TAB + 5 * 16 - 4), dict(tab=a + 6 * M + 16),   # a column destination on the table
            dict(old=a + 6 * M + 16))                                             # two destinations on one another


def test_frame_table_planes_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses.  Pool: rows = 9 (hist 3 + 6 steps) of 3 envs, C = 4, a table of n = 5 samples."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    rows, envs = 9, 3
    samples = (rows - 3) * envs

    def table(rows=rows, envs=envs, hist=3, age=AGE, C=4, idx=IDX, first=0, n=5, tab=TAB, af=AF, **kw):
        c = dict(COLS, **kw)
        return lib.ddrl_op_frame_table_planes(rows, envs, hist, age, C, idx, first, n, tab, c["ac"], c["ol"], c["ad"], c["re"], c["acd"],
                                              c["old"], c["add"], c["red"], af, None)

    for kw in shared_refusals(samples) + (
            dict(age=None), dict(envs=0), dict(hist=2), dict(hist=0), dict(rows=3), dict(rows=2), dict(rows=0),   # hist >= C - 1, rows > hist
            dict(rows=2 ** 31 - 1, envs=2 ** 31 - 1), dict(rows=2 ** 16, envs=2 ** 15),   # the plane count does not fit an int32 entry
            dict(tab=AGE - 5 * 16 + 4), dict(tab=AGE + 16), dict(add=AGE + 16)):  # a destination on the age bytes
        assert table(**kw) == INVALID, kw
    assert table(**NO_COLS, tab=None) == INVALID and table(**NO_COLS, age=None) == INVALID   # still checked with the columns left out
    for C in (0, -1, 5, 8, 16):
        assert table(C=C) == UNSUPPORTED and table(C=C, tab=None) == UNSUPPORTED


def test_frame_table_stacks_argument_checks_come_before_hip():
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    samples = 18

    def table(n_rows=samples, C=4, idx=IDX, first=0, n=5, tab=TAB, af=AF, **kw):
        c = dict(COLS, **kw)
        return lib.ddrl_op_frame_table_stacks(n_rows, C, idx, first, n, tab, c["ac"], c["ol"], c["ad"], c["re"], c["acd"], c["old"],
                                              c["add"], c["red"], af, None)

    for kw in shared_refusals(samples) + (dict(n_rows=0), dict(n_rows=-3), dict(n_rows=2 ** 29), dict(n_rows=2 ** 40)):   # n_rows * C planes
        assert table(**kw) == INVALID, kw
    assert table(n_rows=2 ** 29, C=3, tab=None) == INVALID
    assert table(**NO_COLS, tab=None) == INVALID
    for C in (0, -1, 5, 8):
        assert table(C=C) == UNSUPPORTED and table(C=C, tab=None) == UNSUPPORTED


def test_ppo_iter_indexed_argument_checks_come_before_hip():
    """The frame source's checks come before the context is touched, the columns' and B < 1 before it is read: a zeroed block of host
    memory stands in for a context, and nothing below gets as far as reading it."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    block = ctypes.create_string_buffer(1 << 16)
    CTX, PL = ctypes.addressof(block), a + 16 * M

    def it(ctx=CTX, planes=PL, n_planes=27, tab=TAB, ac=COLS["ac"], ol=COLS["ol"], ad=COLS["ad"], re=COLS["re"], B=5, Bg=5):
        return lib.ddrl_ppo_iter_indexed(ctx, planes, n_planes, tab, ac, ol, ad, re, B, Bg, None)

    for kw in (dict(planes=None), dict(planes=PL + 8), dict(planes=PL + 4), dict(planes=PL + 1), dict(tab=None), dict(tab=TAB + 2),
               dict(tab=TAB + 1), dict(n_planes=0), dict(n_planes=-1), dict(n_planes=2 ** 62), dict(ctx=None),
               dict(ac=None), dict(ol=None), dict(ad=None), dict(re=None), dict(B=0), dict(B=-4)):
        assert it(**kw) == INVALID, kw


# ---- the knob -------------------------------------------------------------------------------------------------------------------------
def _configs(network_type="ppo", **options):
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": 4, "discrete_action": True,
           "discrete_actions": list(range(6)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg_nn = ConfigNN(env)
    cfg_nn.NETWORK_TYPE = network_type
    for k, v in options.items():
        setattr(cfg_nn, k, v)
    return {"config": BaseConfig(types.SimpleNamespace(task="in_place", ip="127.0.0.1"), env), "config_nn": cfg_nn, "config_env": env}


def test_knob_parsing_and_default():
    from ddrl4nav_amd.nn import minibatch as M_
    ns = types.SimpleNamespace
    assert M_.frames_in_place_option(ns()) is False and M_.frames_in_place_option(ns(FRAMES_IN_PLACE=False)) is False
    assert M_.frames_in_place_option(ns(FRAMES_IN_PLACE=True)) is True
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="FRAMES_IN_PLACE"):
            M_.frames_in_place_option(ns(FRAMES_IN_PLACE=bad))
    assert not hasattr(_configs()["config_nn"], "FRAMES_IN_PLACE")            # the ConfigNN contract does not carry it
    assert "FRAMES_IN_PLACE" not in M_.KNOBS                                    # it does not bring PPO.learn to the minibatch loop
    assert M_.minibatch_options(ns(FRAMES_IN_PLACE=True)) == M_.DEFAULTS
    M_.refuse_frames_in_place(ns(), "anyone")
    M_.refuse_frames_in_place(ns(FRAMES_IN_PLACE=False), "anyone")


def test_generic_ppo_and_gail_refuse_the_knob():
    from ddrl4nav_amd.nn.generic import GenericPPO
    from ddrl4nav_amd.runner import create_net
    c = _configs(FRAMES_IN_PLACE=True)
    with pytest.raises(ValueError, match="FRAMES_IN_PLACE is built for the Atari fast path alone"):
        GenericPPO(None, None, None, None, c["config"], c["config_nn"])
    with pytest.raises(ValueError, match="FRAMES_IN_PLACE is built for the Atari fast path alone"):
        create_net(_configs("gail", SHARE_CNN_NET=True, FRAMES_IN_PLACE=True), max_batch=8)
    with pytest.raises(ValueError, match="FRAMES_IN_PLACE is built for the Atari fast path alone"):
        from ddrl4nav_amd.nn.gail import GAIL
        GAIL(None, types.SimpleNamespace(config=c["config"], config_nn=c["config_nn"], device="cpu"), None)
    with pytest.raises(ValueError, match="PPO_MINIBATCHES"):                   # the existing guard keeps its own message
        c2 = _configs(FRAMES_IN_PLACE=True, PPO_MINIBATCHES=2)
        GenericPPO(None, None, None, None, c2["config"], c2["config_nn"])
