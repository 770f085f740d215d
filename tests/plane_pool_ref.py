"""What tests/test_plane_pool_*.py share: the age rule and the reconstruction rule of the single-frame pool (include/ddrl.h
ddrl_op_frame_age / ddrl_op_gather_frame_stacks; csrc/fpool.hip) in numpy, and a host model of PlaneRollout's pool built from them.
test_plane_pool_cpu.py checks both rules against the literal deque model of FrameStackWrapper (test_frame_stack_cpu.DequeStack)."""
import numpy as np

PLANE = 84 * 84


def next_age(prev, reset, C):
    """age[i] = 0 where reset[i] != 0, else min(prev[i] + 1, C - 1).  reset None: no env is reset; prev None: every env is."""
    if prev is None:
        assert reset is not None
        return np.zeros(len(reset), np.uint8)
    a = np.minimum(np.asarray(prev, np.int64) + 1, C - 1)
    if reset is not None:
        a = np.where(np.asarray(reset) != 0, 0, a)
    return a.astype(np.uint8)


def source_rows(age, C, hist, n_envs, samples, n_samples=None):
    """(rows [n, C], envs [n], ok [n]): pool row of every channel of the samples b = t * n_envs + i,
    row = hist + t - min(C - 1 - c, age[b], hist + t); ok False (and row 0) outside [0, n_samples)."""
    age = np.asarray(age).reshape(-1)
    n_samples = age.size if n_samples is None else n_samples
    b = np.asarray(samples, np.int64)
    ok = (b >= 0) & (b < n_samples)
    safe = np.where(ok, b, 0)
    t, env = safe // n_envs, safe % n_envs
    newest = hist + t
    back = np.minimum(np.minimum((C - 1 - np.arange(C))[None, :], age[safe].astype(np.int64)[:, None]), newest[:, None])
    return np.where(ok[:, None], newest[:, None] - back, 0), env, ok


def reconstruct(planes, age, C, samples, hist=None, n_samples=None):
    """uint8 [n, C, 84, 84]: the stacks of `samples` from planes [rows, N, 84, 84] and age [rows - hist, N]; zeros where out of range."""
    hist = C - 1 if hist is None else hist
    n_envs = planes.shape[1]
    rows, env, ok = source_rows(age, C, hist, n_envs, samples, n_samples)
    assert rows.min() >= 0 and rows.max() < planes.shape[0]
    out = planes[rows, env[:, None]]
    return np.where(ok[:, None, None, None], out, 0).astype(np.uint8)


class PoolModel:
    """PlaneRollout's pool on the host: put(t, frames, reset) / carry_over() / stacks(t)."""

    def __init__(self, N, T, C, fill=0):
        self.N, self.T, self.C, self.H = N, T, C, C - 1
        self.planes = np.full((self.H + T + 1, N, 84, 84), fill, np.uint8)
        self.age = np.zeros((T + 1, N), np.uint8)

    def put(self, t, frames, reset):
        """reset: True (every env), None (none) or flags [N]."""
        self.planes[self.H + t] = frames
        if t == 0:
            assert reset is True
        flags = np.ones(self.N, np.uint8) if reset is True else reset
        self.age[t] = next_age(self.age[t - 1] if t > 0 else None, flags, self.C)

    def carry_over(self):
        T, H = self.T, self.H
        self.planes[:H + 1] = self.planes[T:T + H + 1].copy()
        self.age[0] = self.age[T]

    def stacks(self, t):
        return reconstruct(self.planes, self.age, self.C, t * self.N + np.arange(self.N))
