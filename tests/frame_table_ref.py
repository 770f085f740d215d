"""What tests/test_in_place_*.py share: the frame tables of include/ddrl.h ddrl_op_frame_table_planes / ddrl_op_frame_table_stacks
(csrc/ftable.hip) in numpy, built on the reconstruction rule of tests/plane_pool_ref.py, and the frames a table names.
test_in_place_cpu.py checks the model against the literal deque model of FrameStackWrapper."""
import numpy as np

import plane_pool_ref as R

PLANE = R.PLANE


def clamp_samples(samples, n_samples):
    """The one difference from the gathers: a sample outside [0, n_samples) is clamped to it before anything is read."""
    return np.clip(np.asarray(samples, np.int64), 0, n_samples - 1)


def _four(e):
    """[n, C] -> int32 [n, 4]: entries c >= C repeat entry C - 1."""
    C = e.shape[1]
    return np.concatenate([e, np.repeat(e[:, C - 1:C], 4 - C, axis=1)], axis=1).astype(np.int32)


def table_planes(age, C, hist, n_envs, samples):
    """int32 [n, 4]: tab[j][c] = pool row * n_envs + env of channel c of the (clamped) sample, rows by plane_pool_ref.source_rows."""
    age = np.asarray(age).reshape(-1)
    b = clamp_samples(samples, age.size)
    rows, env, ok = R.source_rows(age, C, hist, n_envs, b)
    assert ok.all()
    return _four(rows * n_envs + env[:, None])


def table_stacks(n_rows, C, samples):
    """int32 [n, 4]: tab[j][c] = b * C + c for the (clamped) sample b of stacked frames [n_rows][C][84][84]."""
    b = clamp_samples(samples, n_rows)
    return _four(b[:, None] * C + np.arange(C)[None, :])


def clamp_table(tab, n_planes):
    """What the indirect conv1 kernels make of a table: every entry clamped to [0, n_planes)."""
    return np.clip(np.asarray(tab, np.int64), 0, n_planes - 1).astype(np.int32)


def frames_of(planes, tab, C):
    """uint8 [n, C, 84, 84]: the frames a table names in `planes` (any leading shape, whole 84 x 84 planes), entries clamped."""
    flat = np.asarray(planes).reshape(-1, 84, 84)
    return flat[clamp_table(tab, flat.shape[0])[:, :C]]
