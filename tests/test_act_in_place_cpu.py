"""Host side of acting in place (ddrl_op_frame_slot's and ddrl_forward_indexed's argument checks; the header; the ACT_IN_PLACE knob and
its guards) and the numpy model of the slot operator the GPU tests lean on (tests/plane_pool_ref.py + tests/frame_table_ref.py) against
the literal deque model of FrameStackWrapper.  No GPU: every refusal below is decided before the first HIP call."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import frame_table_ref as F
import plane_pool_ref as R
from test_frame_stack_cpu import episode      # the literal deque model of FrameStackWrapper (DequeStack) run over an episode
from test_in_place_cpu import _configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddrl_forward_indexed", "ddrl_op_frame_slot")
INVALID, UNSUPPORTED = -1, -2


# ---- the numpy model of the slot operator ------------------------------------------------------------------------------------------------
def slot_model(prev_age, reset, C, hist, t, n_envs):
    """(age uint8 [n_envs], tab int32 [n_envs, 4]) of ddrl_op_frame_slot: the age rule, then the table rule on the new age row with
    first = t * n_envs, n = n_envs."""
    age = R.next_age(prev_age, reset, C)
    newest = hist + t
    back = np.minimum(np.minimum((C - 1 - np.arange(C))[None, :], age.astype(np.int64)[:, None]), newest)
    e = (newest - back) * n_envs + np.arange(n_envs)[:, None]
    return age, np.concatenate([e, np.repeat(e[:, C - 1:C], 4 - C, axis=1)], axis=1).astype(np.int32)


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_slot_model_names_the_deque_models_frames(C):
    """40 steps of 5 envs with random resets, the slot operator chained step by step: the planes each step's table names are the deque's
    observation of that step, and age and table equal the two models they fuse."""
    n, steps = 5, 40
    stacks, newest, dones = episode(np.random.default_rng(900 + C), n, C, steps)
    assert dones.any() and not dones.all()
    H = C - 1
    planes = np.concatenate([np.full((H, n, 84, 84), 0xEE, np.uint8), newest])
    ages = np.zeros((steps + 1, n), np.uint8)
    for t in range(steps + 1):
        prev, reset = (None, np.ones(n, np.uint8)) if t == 0 else (ages[t - 1], dones[t - 1])
        ages[t], tab = slot_model(prev, reset, C, H, t, n)
        assert np.array_equal(ages[t], R.next_age(prev, reset, C))
        assert tab.shape == (n, 4) and tab.dtype == np.int32 and tab.min() >= 0 and tab.max() < planes.shape[0] * n
        assert np.array_equal(tab, F.table_planes(ages[:t + 1], C, H, n, t * n + np.arange(n))), t
        assert (tab[:, C - 1:] == tab[:, C - 1:C]).all()
        assert np.array_equal(F.frames_of(planes, tab, C), stacks.reshape(steps + 1, n, C, 84, 84)[t]), t
    # a hostile previous age at the first row of a pool without spare history: no entry below 0
    age, tab = slot_model(np.full(n, 255, np.uint8), np.zeros(n, np.uint8), C, C - 1, 0, n)
    assert (age == C - 1).all() and tab.min() >= 0 and np.array_equal(tab[:, 0], np.arange(n))


# ---- header, binding, library ----------------------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_binds():
    from ddrl4nav_amd import _lib, ops
    from ddrl4nav_amd.engine import HotPath
    text = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    for name in NEW:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [13, 10]
    assert re.search(r"#define\s+DDRL_ABI_VERSION\s+3\b", text) and _lib.ABI_VERSION == 3      # additive
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW) and lib.ddrl_abi_version() == 3
    assert callable(ops.frame_slot) and callable(HotPath.forward_indexed)


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
a, M = 0x100000, 0x100000
PREV, RESET, AGE, TAB = a, a + M, a + 2 * M, a + 3 * M


def test_frame_slot_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses.  Pool: rows = 9 (hist 3 + 6 steps) of 5 envs, C = 4, step t = 2."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()

    def slot(rows=9, envs=5, hist=3, C=4, t=2, prev=PREV, reset=RESET, age=AGE, tab=TAB):
        return lib.ddrl_op_frame_slot(rows, envs, hist, C, t, prev, reset, age, tab, None)

    for kw in (dict(age=None), dict(tab=None), dict(prev=None, reset=None), dict(envs=0), dict(envs=-2),
               dict(hist=2), dict(hist=0),                                        # hist >= C - 1
               dict(t=-1), dict(t=6), dict(t=2 ** 31 - 1), dict(rows=5), dict(rows=0),   # 0 <= t, hist + t < rows
               dict(tab=TAB + 4), dict(tab=TAB + 8), dict(tab=TAB + 2), dict(tab=TAB + 1),   # an env's entries are one 16-byte store
               dict(rows=2 ** 16, envs=2 ** 15),                                  # the plane count does not fit an int32 entry
               dict(age=PREV), dict(age=PREV + 4), dict(age=PREV - 4), dict(age=RESET), dict(age=RESET + 4),   # age on what is read
               dict(tab=PREV), dict(tab=PREV - 5 * 16 + 16), dict(tab=RESET - 16), dict(tab=RESET),             # the table on it
               dict(tab=AGE), dict(tab=AGE - 64), dict(age=TAB + 5 * 16 - 1)):    # the two destinations on one another
        assert slot(**kw) == INVALID, kw
    assert slot(prev=None, tab=None) == INVALID and slot(reset=None, age=None) == INVALID      # still checked in the NULL forms
    for C in (0, -1, 5, 8, 16):
        assert slot(C=C) == UNSUPPORTED and slot(C=C, tab=None) == UNSUPPORTED


def test_forward_indexed_argument_checks_come_before_hip():
    """The frame source's checks come before the context is touched, a missing value pointer and n < 1 before it is read: a zeroed
    block of host memory stands in for a context, and nothing below gets as far as reading it."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    block = ctypes.create_string_buffer(1 << 16)
    CTX, PL, OUT = ctypes.addressof(block), a + 16 * M, a + 20 * M

    def fwd(ctx=CTX, planes=PL, n_planes=27, tab=TAB, n=5, value=OUT):
        return lib.ddrl_forward_indexed(ctx, planes, n_planes, tab, n, None, 1, 2, OUT + M, value, OUT + 2 * M, OUT + 3 * M, None)

    for kw in (dict(planes=None), dict(planes=PL + 8), dict(planes=PL + 4), dict(planes=PL + 1), dict(tab=None), dict(tab=TAB + 2),
               dict(tab=TAB + 1), dict(n_planes=0), dict(n_planes=-1), dict(n_planes=2 ** 62), dict(n_planes=(2 ** 63 - 1) // 7056 + 1),
               dict(ctx=None), dict(value=None), dict(n=0), dict(n=-4)):
        assert fwd(**kw) == INVALID, kw
    # the frame source is refused even where everything else is missing too
    assert fwd(ctx=None, planes=PL + 8) == INVALID and fwd(ctx=None, value=None, tab=None) == INVALID


# ---- the knob -------------------------------------------------------------------------------------------------------------------------
def test_knob_parsing_and_default():
    from ddrl4nav_amd.nn import minibatch as M_
    ns = types.SimpleNamespace
    assert M_.act_in_place_option(ns()) is False and M_.act_in_place_option(ns(ACT_IN_PLACE=False)) is False
    assert M_.act_in_place_option(ns(ACT_IN_PLACE=True)) is True
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="ACT_IN_PLACE"):
            M_.act_in_place_option(ns(ACT_IN_PLACE=bad))
    assert not hasattr(_configs()["config_nn"], "ACT_IN_PLACE")               # the ConfigNN contract does not carry it
    assert "ACT_IN_PLACE" not in M_.KNOBS and M_.minibatch_options(ns(ACT_IN_PLACE=True)) == M_.DEFAULTS
    # the two in-place knobs are apart: either leaves the other at its default
    assert M_.act_in_place_option(ns(FRAMES_IN_PLACE=True)) is False and M_.frames_in_place_option(ns(ACT_IN_PLACE=True)) is False
    M_.refuse_act_in_place(ns(), "anyone")
    M_.refuse_act_in_place(ns(ACT_IN_PLACE=False), "anyone")
    M_.refuse_act_in_place(ns(FRAMES_IN_PLACE=True), "anyone")


def test_generic_ppo_and_gail_refuse_the_knob():
    from ddrl4nav_amd.nn.generic import GenericPPO
    from ddrl4nav_amd.runner import create_net
    c = _configs(ACT_IN_PLACE=True)
    with pytest.raises(ValueError, match="ACT_IN_PLACE is built for the Atari fast path alone"):
        GenericPPO(None, None, None, None, c["config"], c["config_nn"])
    with pytest.raises(ValueError, match="ACT_IN_PLACE is built for the Atari fast path alone"):
        create_net(_configs("gail", SHARE_CNN_NET=True, ACT_IN_PLACE=True), max_batch=8)
    with pytest.raises(ValueError, match="ACT_IN_PLACE is built for the Atari fast path alone"):
        from ddrl4nav_amd.nn.gail import GAIL
        GAIL(None, types.SimpleNamespace(config=c["config"], config_nn=c["config_nn"], device="cpu"), None)
    with pytest.raises(ValueError, match="ACT_IN_PLACE must be True or False"):
        c2 = _configs(ACT_IN_PLACE=1)
        GenericPPO(None, None, None, None, c2["config"], c2["config_nn"])


def test_plane_rollout_argument_overrides_the_nets_value(monkeypatch):
    """PlaneRollout(act_in_place=None) follows the net; True / False override it.  The constructor is run with the allocations stubbed
    out (no device here): what is looked at is which buffers it asks for."""
    import torch
    from ddrl4nav_amd.agent import plane_rollout as P
    from ddrl4nav_amd.agent import rollout as R
    asked = []

    class FakeTensor:
        def __init__(self, shape, dtype):
            self.shape, self.dtype = tuple(shape), dtype

        def __getitem__(self, k):
            return self

    def alloc(shape, dtype=None, device=None):
        asked.append((tuple(shape), dtype))
        return FakeTensor(shape, dtype)

    fake_torch = types.SimpleNamespace(empty=alloc, zeros=alloc, ones=alloc, uint8=torch.uint8, float32=torch.float32, int32=torch.int32,
                                       device=lambda d: d, cuda=types.SimpleNamespace(Stream=lambda device=None: None))
    monkeypatch.setattr(P, "torch", fake_torch)
    monkeypatch.setattr(R, "torch", fake_torch)     # the constructor's shared part lives in agent/rollout.py
    N, T, C = 5, 6, 4

    def build(net_value, arg):
        del asked[:]
        net = types.SimpleNamespace(device="cpu", n_actions=6)
        if net_value is not None:
            net.act_in_place = net_value
        ro = P.PlaneRollout(net, N, horizon=T, channels=C, act_in_place=arg)
        return ro, list(asked)

    stack, tab = ((N, C, 84, 84), torch.uint8), ((N, 4), torch.int32)
    for net_value, arg, want in ((None, None, False), (False, None, False), (True, None, True), (True, False, False), (False, True, True),
                                 (None, True, True)):
        ro, shapes = build(net_value, arg)
        assert ro.act_in_place is want, (net_value, arg)
        assert (stack in shapes) == (not want) and (tab in shapes) == want, (net_value, arg)
        assert (ro._stack is None) == want and (ro._slot_tab is None) == (not want) and ro._slot_t == -1
