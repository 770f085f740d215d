"""Host side of the single-frame experience pool (csrc/fpool.hip's argument checks; the header; data.FramePlanes and
agent.PlaneRollout's guards) and the numpy model the GPU tests lean on (tests/plane_pool_ref.py) against the literal deque model of
FrameStackWrapper.  No GPU: every refusal below is decided before the first HIP call."""
import os
import re
import types

import numpy as np
import pytest
import torch

import plane_pool_ref as R
from test_frame_stack_cpu import episode      # the literal deque model of FrameStackWrapper (DequeStack) run over an episode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddrl_op_frame_age", "ddrl_op_gather_frame_stacks")
INVALID, UNSUPPORTED = -1, -2
PLANE = R.PLANE


# ---- the numpy model against the deque ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_age_and_reconstruction_rules_equal_the_deque_model(C):
    """40 steps of 5 envs with random resets: planes stored once + the age rule give the deque's observation at every step."""
    n, steps = 5, 40
    stacks, newest, dones = episode(np.random.default_rng(300 + C), n, C, steps)
    assert dones.any() and not dones.all()
    H = C - 1
    planes = np.concatenate([np.full((H, n, 84, 84), 0xEE, np.uint8), newest])      # the history rows are never read
    age = np.zeros((steps + 1, n), np.uint8)
    age[0] = R.next_age(None, np.ones(n, np.uint8), C)
    for t in range(steps):
        age[t + 1] = R.next_age(age[t], dones[t], C)
    assert age.max() == C - 1 and (age[1:][dones != 0] == 0).all()
    got = R.reconstruct(planes, age, C, np.arange((steps + 1) * n))
    assert np.array_equal(got.reshape(stacks.shape), stacks)
    # age is the deque's own bookkeeping: appends since the last reset, saturated
    since = np.zeros(n, np.int64)
    for t in range(steps):
        since = np.where(dones[t] != 0, 0, since + 1)
        assert np.array_equal(age[t + 1], np.minimum(since, C - 1))


def test_age_rule_null_forms_and_saturation():
    prev = np.array([0, 1, 2, 3, 200, 255], np.uint8)
    reset = np.array([0, 9, 0, 0, 0, 1], np.uint8)
    assert R.next_age(prev, None, 4).tolist() == [1, 2, 3, 3, 3, 3]
    assert R.next_age(prev, reset, 4).tolist() == [1, 0, 3, 3, 3, 0]
    assert R.next_age(prev, reset, 1).tolist() == [0] * 6
    assert R.next_age(None, reset, 4).tolist() == [0] * 6


@pytest.mark.parametrize("C", [2, 4])
def test_pool_model_carries_history_across_rollouts(C):
    """PoolModel over three chained rollouts equals one long deque episode: stacks right after carry_over() read the history rows."""
    N, T = 3, 5
    stacks, newest, dones = episode(np.random.default_rng(7 + C), N, C, 3 * T, p_done=0.25)
    m = R.PoolModel(N, T, C, fill=0xEE)
    for r in range(3):
        for t in range(T + 1):
            g = r * T + t
            if t > 0 or r == 0:
                m.put(t, newest[g], True if g == 0 else dones[g - 1])
            assert np.array_equal(m.stacks(t), stacks[g]), (r, t)
        m.carry_over()


def test_hostile_age_is_clamped_to_the_pool():
    """255 in every age byte: the look-back is min(C - 1 - c, hist + t) -- never a row below 0, never above the sample's own."""
    C, N, T = 4, 3, 5
    age = np.full((T + 1, N), 255, np.uint8)
    rows, env, ok = R.source_rows(age, C, 0, N, np.arange((T + 1) * N))          # hist = 0 makes the clamp bite at t < C - 1
    assert ok.all() and rows.min() == 0
    t = np.arange((T + 1) * N) // N
    assert np.array_equal(rows, np.maximum(t[:, None] - (C - 1 - np.arange(C))[None, :], 0))
    rows3, _, _ = R.source_rows(age, C, C - 1, N, np.arange((T + 1) * N))
    assert np.array_equal(rows3, t[:, None] + np.arange(C)[None, :])                # with C - 1 history rows: the plain shifted window


# ---- header, binding, library ----------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    from ddrl4nav_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    for name in NEW:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    assert len(_lib.SIGNATURES["ddrl_op_frame_age"][1]) == 6 and len(_lib.SIGNATURES["ddrl_op_gather_frame_stacks"][1]) == 20
    declared = set(re.findall(r"int32_t\s+(ddrl_\w+)\s*\(", text)) | {"ddrl_status_string"}
    assert set(_lib.SIGNATURES) <= declared
    assert re.search(r"#define\s+DDRL_ABI_VERSION\s+3\b", text) and _lib.ABI_VERSION == 3
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW) and lib.ddrl_abi_version() == 3
    assert callable(ops.frame_age) and callable(ops.gather_frame_stacks)


def test_a_library_built_before_the_pool_gets_the_rebuild_hint():
    from ddrl4nav_amd import _lib

    class Old:
        def __init__(self, names):
            self.ddrl_abi_version = lambda: 3
            for n in names:
                setattr(self, n, types.SimpleNamespace())

    names = [n for n in _lib.SIGNATURES if n not in ("ddrl_abi_version",) + NEW]
    with pytest.raises(_lib.DdrlError, match=r"does not export ddrl_op_frame_age, ddrl_op_gather_frame_stacks.*rebuild with `make"):
        _lib._bind(Old(names))


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
def test_frame_age_argument_checks_come_before_hip():
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    a, M = 0x100000, 0x100000
    call = lambda prev=a, reset=a + M, n=64, C=4, age=a + 2 * M: lib.ddrl_op_frame_age(prev, reset, n, C, age, None)
    for kw in (dict(age=None), dict(n=0), dict(n=-5), dict(prev=None, reset=None),
               dict(age=a), dict(age=a + 63), dict(age=a - 63), dict(age=a + M), dict(age=a + M + 63), dict(prev=None, age=a + M - 63)):
        assert call(**kw) == INVALID, kw
    for C in (0, -1, 5, 8):
        assert call(C=C) == UNSUPPORTED and call(C=C, age=None) == UNSUPPORTED


def test_gather_frame_stacks_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses.  Pool: rows = 9 (hist 3 + 6 steps) of 3 envs, C = 4, n = 5 samples gathered."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    a, M = 0x100000, 0x100000
    cols = dict(ac=a + 2 * M, ol=a + 3 * M, ad=a + 4 * M, re=a + 5 * M, acd=a + 6 * M, old=a + 7 * M, add=a + 8 * M, red=a + 9 * M)
    PL, AGE, IDX, AF, DST = a + 16 * M, a + 11 * M, a + M, a + 10 * M, a + 24 * M
    rows, envs = 9, 3
    samples = (rows - 3) * envs                                                 # 18 entries in age and in every column

    def gather(pl=PL, rows=rows, envs=envs, hist=3, age=AGE, C=4, idx=IDX, first=0, n=5, dst=DST, af=AF, **kw):
        c = dict(cols, **kw)
        return lib.ddrl_op_gather_frame_stacks(pl, rows, envs, hist, age, C, idx, first, n, dst, c["ac"], c["ol"], c["ad"], c["re"], c["acd"],
                                               c["old"], c["add"], c["red"], af, None)

    stack_b = 5 * 4 * PLANE
    for kw in (dict(pl=None), dict(age=None), dict(dst=None), dict(n=0), dict(n=-1), dict(envs=0),
               dict(hist=2), dict(hist=0), dict(rows=3), dict(rows=2), dict(rows=0),   # hist >= C - 1, rows > hist
               dict(pl=PL + 8), dict(dst=DST + 4), dict(idx=IDX + 2), dict(af=AF + 1),
               dict(idx=None, first=2 ** 63 - 3),                                  # first + n past int64
               dict(n=2 ** 30), dict(n=2 ** 31 - 1),                               # n * C workgroups do not fit a grid
               dict(rows=2 ** 31 - 1, envs=2 ** 31 - 1),                           # the pool's byte count does not fit
               dict(ac=None), dict(acd=None), dict(ol=None), dict(old=None), dict(ad=None), dict(add=None), dict(re=None), dict(red=None),
               dict(ac=a + 2 * M + 2), dict(red=a + 9 * M + 1),
               dict(ad=None, add=None),                                              # an affine without the advantage column
               dict(dst=PL + PLANE), dict(dst=PL + rows * envs * PLANE - 16),        # stacks_dst inside the planes
               dict(pl=DST + stack_b - 16),                                          # the planes begin inside stacks_dst
               dict(dst=AGE - stack_b + 16), dict(add=AGE + 16),            # a destination on the age bytes
               dict(acd=a + 2 * M + 4), dict(old=a + 4 * M + 4 * samples - 4), dict(red=a + 5 * M),   # ... on a source column
               dict(add=IDX + 16), dict(add=AF + 4),                                 # ... on the indices, on the affine pair
               dict(acd=PL + 64), dict(red=DST + stack_b - 4),                       # ... inside the planes, at the end of stacks_dst
               dict(old=a + 6 * M + 16)):                                            # two destinations on one another
        assert gather(**kw) == INVALID, kw
    none = dict(ac=None, acd=None, ol=None, old=None, ad=None, add=None, re=None, red=None, af=None)
    assert gather(**none, pl=None) == INVALID and gather(**none, idx=None, dst=PL) == INVALID   # still checked with the columns left out
    for C in (0, -1, 5, 8, 16):
        assert gather(C=C) == UNSUPPORTED and gather(C=C, pl=None) == UNSUPPORTED


# ---- FramePlanes / PlaneRollout guards -------------------------------------------------------------------------------------------------
def _planes(T=5, N=3, C=4):
    return torch.zeros((C - 1 + T + 1, N, 84, 84), dtype=torch.uint8), torch.zeros((T + 1, N), dtype=torch.uint8)


def test_frame_planes_shape_and_range_guards():
    from ddrl4nav_amd.data import Experience, FramePlanes
    p, a = _planes()
    fp = FramePlanes(p, a, 5, 3, 4)
    assert len(fp) == 15 and fp.shape == (15, 4, 84, 84) and len(Experience(states=[fp])) == 15
    for bad in (lambda: FramePlanes(p[1:], a, 5, 3, 4), lambda: FramePlanes(p, a[1:], 5, 3, 4), lambda: FramePlanes(p, a, 5, 3, 5),
                lambda: FramePlanes(p, a, 5, 3, 0), lambda: FramePlanes(p.float(), a, 5, 3, 4), lambda: FramePlanes(p, a, 6, 3, 3)):
        with pytest.raises(ValueError):
            bad()
    for lo, hi in ((-1, 3), (3, 3), (5, 2), (0, 16), (15, 16)):                     # row T is not part of the batch
        with pytest.raises(ValueError, match="batch of 15"):
            fp.stacks(lo, hi)


def test_generic_ppo_and_gail_refuse_frame_planes():
    """The check is the first statement of both learn generators: it needs no net."""
    from ddrl4nav_amd.data import Experience, FramePlanes
    from ddrl4nav_amd.nn.gail import GAIL
    from ddrl4nav_amd.nn.generic import GenericPPO
    exp = Experience(states=[FramePlanes(*_planes(), 5, 3, 4)])
    for cls in (GenericPPO, GAIL):
        with pytest.raises(TypeError, match="Atari fast path alone"):
            next(cls.learn(types.SimpleNamespace(), exp))


def test_plane_rollout_guards():
    from ddrl4nav_amd.agent import DeviceRollout, PlaneRollout
    assert issubclass(PlaneRollout, DeviceRollout)
    fake = types.SimpleNamespace(device="cpu", n_actions=6)
    with pytest.raises(ValueError, match="horizon 3 < channels 4"):
        PlaneRollout(fake, 3, horizon=3, channels=4)                            # refused before anything is allocated
    with pytest.raises(ValueError, match="1 to 4"):
        PlaneRollout(fake, 3, horizon=8, channels=5)
    ro = PlaneRollout.__new__(PlaneRollout)
    ro.t0, ro.N, ro.C, ro.H, ro.T = 0, 3, 4, 3, 5
    for put in (lambda: ro.put_frames(0, None), lambda: ro.put_frames_from_ring(0, None)):
        with pytest.raises(ValueError, match="DeviceRollout"):
            put()
    f = torch.zeros((3, 84, 84), dtype=torch.uint8)
    for reset in (None, False, torch.ones(3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="slot 0 has no previous stack"):
            ro.put_new_frames(0, f, reset=reset)
        with pytest.raises(ValueError, match="slot 0 has no previous stack"):
            ro.put_new_frames_from_ring(0, None, reset=reset)                   # refused before the ring is touched
    ro.t0 = 1
    with pytest.raises(ValueError, match="carried over"):
        ro.put_new_frames(0, f, reset=True)
