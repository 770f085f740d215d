"""Single-frame ingest without a GPU: the yardstick the GPU tests lean on (a literal restatement of the reference's
FrameStackWrapper, USTC_lab/env/gym_env/wrapper/warputils.py:112-131: one deque(maxlen=C) of single frames per env) against the closed
form ddrl_frame_stack_push implements, and the entry point's argument checks, which run before anything touches HIP.  Everything is
uint8 and compared exactly."""
import collections
import ctypes

import numpy as np
import pytest

from ddrl4nav_amd import _lib

PLANE = 84 * 84
INVALID_ARG, UNSUPPORTED = -1, -2


class DequeStack:
    """FrameStackWrapper for n envs: reset = C appends of the first frame, step = one append; the observation is the deque's
    frames oldest first, [C, 84, 84] per env."""

    def __init__(self, n, channels):
        self.q = [collections.deque(maxlen=channels) for _ in range(n)]
        self.C = channels

    def reset(self, i, frame):
        for _ in range(self.C):
            self.q[i].append(frame)

    def step(self, i, frame):
        self.q[i].append(frame)

    def obs(self):
        return np.stack([np.stack(list(q), axis=0) for q in self.q], axis=0)


def closed_form(prev, newest, reset):
    """The formula of include/ddrl.h (ddrl_frame_stack_push) in numpy."""
    n, C = prev.shape[:2]
    nxt = np.empty_like(prev)
    for i in range(n):
        for c in range(C):
            if reset is not None and reset[i] != 0:
                nxt[i, c] = newest[i]
            elif c < C - 1:
                nxt[i, c] = prev[i, c + 1]
            else:
                nxt[i, c] = newest[i]
    return nxt


def episode(rng, n, channels, steps, p_done=0.3):
    """A synthetic episode through the deque model: (stacks [steps+1, n, C, 84, 84], newest [steps+1, n, 84, 84], dones [steps, n]).
    dones[t] ends env i's episode at step t: its observation t+1 is the first of a new one (NeverStopWrapper.step resets)."""
    model = DequeStack(n, channels)
    newest = rng.integers(0, 256, size=(steps + 1, n, 84, 84), dtype=np.uint8)
    dones = (rng.random((steps, n)) < p_done).astype(np.uint8)
    for i in range(n):
        model.reset(i, newest[0, i])
    stacks = [model.obs()]
    for t in range(steps):
        for i in range(n):
            (model.reset if dones[t, i] else model.step)(i, newest[t + 1, i])
        stacks.append(model.obs())
    return np.stack(stacks), newest, dones


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_closed_form_equals_the_deque_model(channels):
    rng = np.random.default_rng(100 + channels)
    stacks, newest, dones = episode(rng, 5, channels, 40)
    assert dones.any() and not dones.all()
    cur = closed_form(np.zeros_like(stacks[0]), newest[0], np.ones(5, np.uint8))   # the first observation: reset everywhere
    assert np.array_equal(cur, stacks[0])
    for t in range(40):
        cur = closed_form(cur, newest[t + 1], dones[t])
        assert np.array_equal(cur, stacks[t + 1]), "step %d" % t
    # no flags at all == all-zero flags
    assert np.array_equal(closed_form(stacks[3], newest[4], None), closed_form(stacks[3], newest[4], np.zeros(5, np.uint8)))


def _push(prev, newest, reset, n, channels, nxt):
    f = _lib.load().ddrl_frame_stack_push
    return f(ctypes.c_void_p(prev), ctypes.c_void_p(newest), ctypes.c_void_p(reset), n, channels, ctypes.c_void_p(nxt), None)


def test_argument_checks_come_before_hip():
    """Fabricated, aligned, non-NULL addresses that are never dereferenced: every refused call returns before the first HIP call, so
    this runs where there is no GPU."""
    n = 4
    prev, newest, reset, nxt = 0x7E0000000000, 0x7E0010000000, 0x7E0020000000, 0x7E0030000000
    stack = n * 4 * PLANE
    assert _push(prev, newest, reset, 0, 4, nxt) == INVALID_ARG
    assert _push(prev, newest, reset, -3, 4, nxt) == INVALID_ARG
    assert _push(None, newest, reset, n, 4, nxt) == INVALID_ARG
    assert _push(None, newest, reset, n, 2, nxt) == INVALID_ARG
    assert _push(prev, None, reset, n, 4, nxt) == INVALID_ARG
    assert _push(prev, newest, reset, n, 4, None) == INVALID_ARG
    assert _push(None, None, reset, n, 1, nxt) == INVALID_ARG          # C = 1 needs no prev, but still a frame
    for off in (1, 4, 8):
        assert _push(prev + off, newest, reset, n, 4, nxt) == INVALID_ARG
        assert _push(prev, newest + off, reset, n, 4, nxt) == INVALID_ARG
        assert _push(prev, newest, reset, n, 4, nxt + off) == INVALID_ARG
    # [prev, prev + n*C*7056) against [next, ...): identical, next inside prev's range from either side, last / first 16 bytes shared
    assert _push(prev, newest, reset, n, 4, prev) == INVALID_ARG
    assert _push(prev, newest, reset, n, 4, prev + 4 * PLANE) == INVALID_ARG
    assert _push(prev, newest, reset, n, 4, prev - 4 * PLANE) == INVALID_ARG
    assert _push(prev, newest, reset, n, 4, prev + stack - 16) == INVALID_ARG
    assert _push(prev, newest, reset, n, 4, prev - stack + 16) == INVALID_ARG
    for channels in (0, -1, 5, 8, 12, 16):
        assert _push(prev, newest, reset, n, channels, nxt) == UNSUPPORTED
        assert _push(prev, newest, None, n, channels, nxt) == UNSUPPORTED


def test_entry_point_is_declared_and_bound():
    assert "ddrl_frame_stack_push" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "ddrl_frame_stack_push")
    assert _lib.load().ddrl_abi_version() == 3      # additive
