"""Float64 NumPy model of the running normalisation (csrc/runnorm.hip, agent/normalize.py, the rollouts' knobs): what the CPU and GPU
tests of tests/test_running_norm_*.py compare against.  No torch, no GPU.

RunningRef restates the update of the reference's RunningMeanStd (USTC_lab/env/gym_env/wrapper/warputils.py:94-109) and is pinned to it
by fixture f28 (tests/golden/make_golden_running_norm.py drives the reference's own class)."""
import numpy as np

U64 = 2.0 ** -53      # unit roundoff of a double
U32 = 2.0 ** -24      # ... of a float


class RunningRef:
    """count, mean[d], var[d] (population variance) in float64; fresh = (0, 0, 1), the reference constructor's defaults."""

    def __init__(self, d):
        self.count, self.mean, self.var = 0.0, np.zeros(d), np.ones(d)

    def copy(self):
        c = RunningRef(len(self.mean))
        c.count, c.mean, c.var = self.count, self.mean.copy(), self.var.copy()
        return c

    def merge(self, n, bm, bv):
        """Chan's parallel update with a batch of n rows whose mean / population variance are bm / bv."""
        if n == 0:
            return self
        delta = bm - self.mean
        tot = self.count + n
        mean = self.mean + delta * n / tot
        var = (self.var * self.count + bv * n + delta ** 2 * self.count * n / tot) / tot
        self.count, self.mean, self.var = tot, mean, var
        return self

    def update(self, x):
        """The reference's update: two-pass batch mean and variance of the rows of x."""
        x = np.asarray(x, np.float64).reshape(len(x), -1)
        return self.merge(float(len(x)), x.mean(axis=0), x.var(axis=0))

    def merge_sums(self, sums):
        """The device's update: the batch as pending sums (n, S1[d], S2[d]); bm = S1 / n, bv = max(0, S2 / n - bm^2)."""
        d = len(self.mean)
        n, s1, s2 = float(sums[0]), np.asarray(sums[1:1 + d], np.float64), np.asarray(sums[1 + d:], np.float64)
        if n == 0:
            return self
        bm = s1 / n
        return self.merge(n, bm, np.maximum(0.0, s2 / n - bm * bm))

    def state(self):
        return np.concatenate([[self.count], self.mean, self.var])


def sums64(x):
    """Pending sums (n, S1[d], S2[d]) of the rows of x, every term and sum in float64."""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    return np.concatenate([[float(len(x))], x.sum(axis=0), (x * x).sum(axis=0)])


def two_pass(x):
    """(mean, population variance) per column, two passes in float64: the reference of the moments bound."""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    return x.mean(axis=0), x.var(axis=0)


def moments_bound(n, mean64, var64):
    """(bound on |mean - mean64|, bound on |var - var64|) of moments formed from double sums of n terms: with gamma = (n + 8) 2^-53,
    4 gamma (|mean64| + std64) and 4 gamma (var64 + mean64^2)."""
    g = (n + 8) * U64
    return 4 * g * (np.abs(mean64) + np.sqrt(var64)), 4 * g * (var64 + mean64 ** 2)


class BoundedRef:
    """The reference's update on a chain of batches, with the distance a state built from DOUBLE SUMS of the same batches may keep from
    it.  Per batch: the batch moments' own bound (moments_bound) enters the mean with a weight n / tot <= 1; the variance takes the
    batch variance with that weight and delta^2 count n / tot^2 <= delta^2 / 4, so an error e of delta costs at most |delta| e / 2 (2
    |delta| e is allowed: both the batch mean and the prior mean carry one); the merge itself is a dozen correctly rounded double
    operations, 1e-14 (|mean| + |bm|) and 1e-14 (var + bv + delta^2).  What the earlier batches left is carried along."""

    def __init__(self, d):
        self.run, self.tol_mean, self.tol_var = RunningRef(d), np.zeros(d), np.zeros(d)

    def update(self, x):
        x = np.asarray(x, np.float64).reshape(len(x), -1)
        if len(x) == 0:
            return self
        bm, bv = two_pass(x)
        e_mean, e_var = moments_bound(len(x), bm, bv)
        delta = np.abs(bm - self.run.mean) if self.run.count else np.zeros(len(bm))
        self.run.update(x)
        self.tol_var = self.tol_var + e_var + 2 * delta * (e_mean + self.tol_mean) + 1e-14 * (self.run.var + bv + delta ** 2)
        self.tol_mean = self.tol_mean + e_mean + 1e-14 * (np.abs(self.run.mean) + np.abs(bm))
        return self

    def check(self, state, factor=1.0, ref=None):
        """state = (count, mean[d], var[d]) of the device; ref: another state to compare with instead of the reference's (factor 2:
        two states that each lie inside the bound)."""
        d = len(self.run.mean)
        state = np.asarray(state, np.float64)
        want = self.run.state() if ref is None else np.asarray(ref, np.float64)
        assert state[0] == want[0] == self.run.count, (state[0], want[0], self.run.count)
        err_mean, err_var = np.abs(state[1:1 + d] - want[1:1 + d]), np.abs(state[1 + d:] - want[1 + d:])
        assert np.all(err_mean <= factor * self.tol_mean), (err_mean, self.tol_mean)
        assert np.all(err_var <= factor * self.tol_var), (err_var, self.tol_var)


def moments_of_sums(sums, d):
    n = float(sums[0])
    mean = np.asarray(sums[1:1 + d], np.float64) / n
    return mean, np.asarray(sums[1 + d:], np.float64) / n - mean * mean


def columns(rng, n, d, ld=None, poison=np.nan):
    """fp32 [n, ld] test matrix: column j = offset_j + scale_j * z_j with z_j a normal sample standardised to mean 0 and std 1 (n > 1)
    and |offset_j| <= 60 scale_j, so that |mean| / std <= 100 holds for every column whatever n; the padding columns [d, ld) poisoned."""
    ld = d if ld is None else ld
    scale = 10.0 ** rng.uniform(-2, 2, size=d)
    offset = scale * rng.uniform(-60, 60, size=d)
    z = rng.standard_normal((n, d))
    if n > 1:
        z = (z - z.mean(axis=0)) / z.std(axis=0)
    x = np.full((n, ld), poison, np.float32)
    x[:, :d] = (offset + scale * z).astype(np.float32)
    return x


# (n, d, ld) of the column-moments tests: the issue's grid, then n and d at each of the kernel's own widths -1, 0, +1 (csrc/runnorm.hip
# moments_grid).  The kernel has seven geometries: lanes = 1, 2, 4, 8, 16, 32, 64 threads along the columns for d <= 4, 8, 16, 32, 64,
# 128 and beyond; a tile is 4 * lanes columns, a slab 4 * phases = 1024 / lanes rows (and grows once n passes 256 slabs: 4097 rows at
# 4 phases).  Per geometry: d on both sides of the tile width, n = slab - 1, slab, slab + 1 (the last one two slabs, the second ragged)
# and an n of two and a half slabs.  Padded and odd strides ride along.
MOMENT_SHAPES = [(1, 1, 1), (7, 5, 5), (64, 1, 1), (513, 3, 8), (257, 960, 960), (33, 6912, 6912),
                 (9, 4, 4), (9, 5, 7), (9, 8, 8), (9, 9, 12), (19, 128, 128), (19, 129, 131),
                 (1023, 1, 1), (1024, 1, 1), (1025, 1, 3), (2561, 3, 3),                  # lanes 1: slabs of 1024 rows
                 (511, 5, 5), (512, 8, 8), (513, 7, 9), (1281, 6, 6),                    # lanes 2: 512 rows, tile 8 (d = 8 | 9)
                 (255, 15, 15), (256, 16, 16), (257, 9, 11), (641, 16, 20),              # lanes 4: 256 rows, tile 16 (d = 16 | 17)
                 (127, 17, 17), (128, 31, 31), (129, 32, 32), (321, 17, 19),             # lanes 8: 128 rows, tile 32 (d = 32 | 33)
                 (63, 33, 33), (64, 63, 63), (65, 64, 64), (161, 64, 68),                # lanes 16: 64 rows, tile 64 (d = 64 | 65)
                 (31, 65, 65), (32, 127, 127), (33, 128, 128), (81, 65, 67),             # lanes 32: 32 rows, tile 128 (d = 128 | 129)
                 (15, 255, 255), (16, 256, 256), (17, 257, 260), (41, 129, 132),         # lanes 64: 16 rows, tile 256 (d = 256 | 257)
                 (4096, 253, 256), (4097, 253, 256)]                                     # 256 slabs, then slabs of 20 rows


def affine_ref(mean, var, eps, center=True):
    """(shift, scale) fp32 [2, d]: shift = float(mean) or 0, scale = float(1 / sqrt(var + eps)) formed in double."""
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    shift = mean.astype(np.float32) if center else np.zeros(mean.shape, np.float32)
    return np.stack([shift.reshape(-1), (1.0 / np.sqrt(var + eps)).astype(np.float32).reshape(-1)])


def normalize_ref(x, affine, clip):
    """fp32: (x - shift) * scale, a subtract and a multiply each rounded to fp32, then v < -clip ? -clip : (v > clip ? clip : v)."""
    x = np.asarray(x, np.float32)
    shape = x.shape
    x = x.reshape(-1, affine.shape[1])
    clip = np.float32(clip)
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((x - affine[0][None, :]).astype(np.float32) * affine[1][None, :]).astype(np.float32)
        v = np.where(v < -clip, -clip, np.where(v > clip, clip, v)).astype(np.float32)
    return v.reshape(shape)


def discounted_ref(rewards, dones, gamma, carry):
    """fp32 loop of ddrl_op_discounted_returns over [T, N]: returns (trace [T, N], carry [N])."""
    rewards = np.asarray(rewards, np.float32)
    gamma = np.float32(gamma)
    c = np.asarray(carry, np.float32).copy()
    trace = np.empty_like(rewards)
    for t in range(rewards.shape[0]):
        g = ((c * gamma).astype(np.float32) + rewards[t]).astype(np.float32)
        trace[t] = g
        c = np.where(np.asarray(dones[t]) != 0, np.float32(0.0), g).astype(np.float32)
    return trace, c


class ObsNormRef:
    """Host replay of one normalised component of StateRollout: put(raw rows) counts them and returns the slot as stored (normalised
    with the affine frozen at the last finish()); finish() commits and freezes."""

    def __init__(self, d, eps=1e-8, clip=10.0, center=True):
        self.d, self.eps, self.clip, self.center = d, eps, clip, center
        self.run = RunningRef(d)
        self.pending = np.zeros(1 + 2 * d)
        self.freeze()

    def freeze(self):
        self.affine = affine_ref(self.run.mean, self.run.var, self.eps, self.center)

    def put(self, raw):
        raw = np.asarray(raw, np.float32).reshape(len(raw), self.d)
        self.pending = self.pending + sums64(raw)
        return normalize_ref(raw, self.affine, self.clip)

    def finish(self):
        self.run.merge_sums(self.pending)
        self.pending = np.zeros(1 + 2 * self.d)
        self.freeze()


class ReturnNormRef:
    """Host replay of normalize_returns: scale(rewards, dones) of a finished rollout -> rewards_norm."""

    def __init__(self, n_envs, gamma, eps=1e-8, clip=10.0):
        self.gamma = np.float32(gamma)
        self.carry = np.zeros(n_envs, np.float32)
        self.norm = ObsNormRef(1, eps, clip, center=False)

    def scale(self, rewards, dones):
        trace, self.carry = discounted_ref(rewards, dones, self.gamma, self.carry)
        self.norm.pending = self.norm.pending + sums64(trace.reshape(-1, 1))
        self.norm.finish()
        return normalize_ref(np.asarray(rewards, np.float32).reshape(-1, 1), self.norm.affine, self.norm.clip).reshape(rewards.shape)
