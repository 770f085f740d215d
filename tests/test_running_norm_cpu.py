"""Host side of the running observation / return normalisation (tests/running_norm_ref.py against the reference's RunningMeanStd;
csrc/runnorm.hip's argument checks; the knobs' validation; the header).  No GPU."""
import os
import re
import types

import numpy as np
import pytest

import running_norm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddrl_op_column_moments_ws_floats", "ddrl_op_column_moments", "ddrl_op_running_merge", "ddrl_op_running_affine",
       "ddrl_op_normalize_columns", "ddrl_op_discounted_returns")


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300))


def test_model_reproduces_the_reference_fixture(golden):
    """Fixture f28: six updates of the reference's own RunningMeanStd (batch sizes 1, 2, 7, 64, 3, 513 over d = 5)."""
    g = golden("f28_running_mean_std")
    assert list(g["batches"]) == [1, 2, 7, 64, 3, 513]
    run = R.RunningRef(5)
    assert run.count == g["count0"] == 0 and np.all(run.mean == g["mean0"]) and np.all(run.var == g["var0"])
    for i, n in enumerate(g["batches"]):
        x = g["x%d" % i]
        assert x.shape == (n, 5) and x.dtype == np.float64 and np.array_equal(x, x.astype(np.float32))
        run.update(x)
        assert run.count == g["count%d" % (i + 1)]
        assert _rel(run.mean, g["mean%d" % (i + 1)]) <= 1e-12 and _rel(run.var, g["var%d" % (i + 1)]) <= 1e-12, i
    assert run.count == 590


def test_pooled_sums_merged_once_equal_the_update_on_the_concatenation(golden):
    """k batches' pending sums added up and merged once against the reference's update on the concatenated rows.  Into a fresh state the
    merge returns the batch moments themselves (count 0: mean = bm, var = bv), so the moments bound applies as it stands.  Into a state
    that holds rows already, the batch moments enter with weights n / tot <= 1 and the variance also through delta^2 count n / tot^2
    <= delta^2 / 4: the bound is that of the moments plus |delta| times the mean's, plus a dozen roundings of the merge itself."""
    g = golden("f28_running_mean_std")
    xs = [g["x%d" % i] for i in range(6)]
    for first in (0, 3):      # fresh state; a state that holds the first three batches
        ref, got = R.RunningRef(5), R.RunningRef(5)
        for x in xs[:first]:
            ref.update(x)
            got.update(x)
        prior = got.copy()
        pooled = sum(R.sums64(x) for x in xs[first:])
        got.merge_sums(pooled)
        cat = np.concatenate(xs[first:])
        ref.update(cat)
        assert got.count == ref.count == 590
        bm, bv = R.two_pass(cat)
        e_mean, e_var = R.moments_bound(len(cat), bm, bv)
        delta = np.abs(bm - prior.mean) if first else 0.0
        slack_mean = 1e-14 * (np.abs(ref.mean) + np.abs(bm)) if first else 0.0
        slack_var = 1e-14 * (ref.var + bv + delta ** 2) if first else 0.0
        assert np.all(np.abs(got.mean - ref.mean) <= e_mean + slack_mean), first
        assert np.all(np.abs(got.var - ref.var) <= e_var + delta * e_mean + slack_var), first


@pytest.mark.parametrize("shape", R.MOMENT_SHAPES)
def test_sum_of_squares_in_double_stays_inside_the_moments_bound(shape):
    """The GPU test compares S1 / n and S2 / n - (S1 / n)^2 of the device's double sums with the two-pass float64 moments inside
    moments_bound.  For its inputs (|mean| / std <= 100) the model's own one-pass evaluation has to stay inside that bound too --
    otherwise the bound would ask more of the kernel than the formula can give."""
    n, d, ld = shape
    x = R.columns(np.random.default_rng(n * 131 + d), n, d, ld)
    assert np.isnan(x[:, d:]).all() and np.isfinite(x[:, :d]).all()
    mean64, var64 = R.two_pass(x[:, :d])
    if n > 1:
        assert np.all(np.abs(mean64) <= 100 * np.sqrt(var64))
    mean, var = R.moments_of_sums(R.sums64(x[:, :d]), d)
    e_mean, e_var = R.moments_bound(n, mean64, var64)
    assert np.all(np.abs(mean - mean64) <= e_mean) and np.all(np.abs(var - var64) <= e_var)


def test_moment_shapes_sit_at_the_kernels_own_widths():
    """MOMENT_SHAPES claims n and d at every slab / tile width of csrc/runnorm.hip; the size query tells the slabs (floats = slabs * 4 d),
    so the claim is checked against the library: at both ends of each geometry's range of d, `slab` rows are one slab and one more row
    two, and the list holds slab - 1, slab, slab + 1 and a longer n for that geometry, and d on both sides of every tile width."""
    from ctypes import byref, c_int64
    from ddrl4nav_amd import _lib
    lib = _lib.load()

    def slabs(n, d):
        f = c_int64()
        assert lib.ddrl_op_column_moments_ws_floats(n, d, byref(f)) == 0 and f.value % (4 * d) == 0
        return f.value // (4 * d)

    geometries = [(1, 4, 1024), (5, 8, 512), (9, 16, 256), (17, 32, 128), (33, 64, 64), (65, 128, 32), (129, 6912, 16)]   # d range, slab
    for lo, hi, slab in geometries:
        for d in (lo, hi):
            assert slabs(slab, d) == 1 and slabs(slab + 1, d) == 2 and slabs(256 * slab, d) == 256 and slabs(256 * slab + 1, d) < 256, (d, slab)
        ns = sorted(n for n, d, _ in R.MOMENT_SHAPES if lo <= d <= hi)
        assert {slab - 1, slab, slab + 1} <= set(ns) and ns[-1] > 2 * slab, (lo, hi, ns)
    ds = {d for _, d, _ in R.MOMENT_SHAPES}
    for tile in (4, 8, 16, 32, 64, 128, 256):
        assert {tile, tile + 1} <= ds and (tile - 1 in ds or tile == 4), tile
    assert len(set(R.MOMENT_SHAPES)) == len(R.MOMENT_SHAPES)


def test_model_merge_cases():
    run = R.RunningRef(2)
    run.merge_sums(np.array([0.0, 5.0, 5.0, 1.0, 1.0]))          # an empty pending batch
    assert run.count == 0 and np.all(run.mean == 0) and np.all(run.var == 1)
    run.merge_sums(R.sums64(np.array([[3.0, -2.0]])))            # the first update, n = 1: mean = the row, var = 0
    assert run.count == 1 and np.array_equal(run.mean, [3.0, -2.0]) and np.array_equal(run.var, [0.0, 0.0])
    run.merge_sums(R.sums64(np.array([[3.0, 0.0], [3.0, 2.0]])))  # a constant column
    assert run.count == 3 and run.mean[0] == 3.0 and run.var[0] == 0.0
    assert abs(run.mean[1]) < 1e-15 and abs(run.var[1] - 8.0 / 3.0) < 1e-14


def test_model_normalize_and_returns():
    aff = R.affine_ref([1.0, 0.0], [4.0, 1.0], 0.0)
    assert aff.dtype == np.float32 and np.array_equal(aff, [[1.0, 0.0], [0.5, 1.0]])
    assert np.array_equal(R.affine_ref([1.0, 0.0], [4.0, 1.0], 0.0, center=False)[0], [0.0, 0.0])
    x = np.array([[21.0, np.inf], [-19.0, -np.inf], [np.nan, 3.0], [1.0, np.nan]], np.float32)
    y = R.normalize_ref(x, aff, 10.0)
    assert np.array_equal(y[:2], [[10.0, 10.0], [-10.0, -10.0]]) and np.isnan(y[2, 0]) and y[2, 1] == 3.0 and np.isnan(y[3, 1])
    assert np.array_equal(R.normalize_ref(x[:2], aff, np.inf), [[10.0, np.inf], [-10.0, -np.inf]])
    r = np.array([[1.0, 1.0], [1.0, 1.0], [1.0, 1.0]], np.float32)
    d = np.array([[0, 1], [0, 1], [1, 0]], np.uint8)
    trace, carry = R.discounted_ref(r, d, 0.5, np.array([2.0, 2.0], np.float32))
    assert np.array_equal(trace, [[2.0, 2.0], [2.0, 1.0], [2.0, 1.0]]) and np.array_equal(carry, [0.0, 1.0])
    a, c1 = R.discounted_ref(r[:1], d[:1], 0.5, np.array([2.0, 2.0], np.float32))      # chained calls = one call
    b, c2 = R.discounted_ref(r[1:], d[1:], 0.5, c1)
    assert np.array_equal(np.concatenate([a, b]), trace) and np.array_equal(c2, carry)


def test_knob_validation():
    """Bad clip / eps and a normalize_obs of the wrong length are refused before anything is allocated (no GPU here)."""
    from ddrl4nav_amd.agent import DeviceRollout, PlaneRollout, RunningNorm, StateRollout
    from ddrl4nav_amd.agent.normalize import check_knobs, obs_norm_flags
    assert check_knobs(0, 5) == (0.0, 5.0) and check_knobs(1e-8, float("inf")) == (1e-8, float("inf"))
    for eps, clip in ((-1e-8, 10.0), (float("nan"), 10.0), (float("inf"), 10.0), (1e-8, 0.0), (1e-8, -1.0), (1e-8, float("nan")),
                      (None, 10.0), (1e-8, "wide")):
        with pytest.raises(ValueError):
            check_knobs(eps, clip)
        with pytest.raises(ValueError):
            RunningNorm((5,), "cuda", eps=eps, clip=clip)
    assert obs_norm_flags(None, 3) == obs_norm_flags(False, 3) == [False] * 3 and obs_norm_flags(True, 2) == [True, True]
    assert obs_norm_flags([True, False, 1], 3) == [True, False, True]
    for bad in ([True], [True] * 4, (), 3):
        with pytest.raises(ValueError):
            obs_norm_flags(bad, 3)
    net = types.SimpleNamespace(device="cuda", n_actions=2, continuous=False)
    shapes = [(1, 960), (5,), (3, 48, 48)]
    for kw in (dict(normalize_obs=[True, False]), dict(normalize_obs=[True] * 4), dict(normalize_obs=True, obs_clip=0.0),
               dict(normalize_obs=True, norm_eps=-1.0), dict(normalize_returns=True, reward_clip=-2.0),
               dict(normalize_returns=True, norm_eps=float("nan"))):
        with pytest.raises(ValueError):
            StateRollout(net, 4, shapes, horizon=3, **kw)
    for cls in (DeviceRollout, PlaneRollout):
        for kw in (dict(reward_clip=0.0), dict(norm_eps=-1e-3)):
            with pytest.raises(ValueError):
                cls(net, 4, horizon=8, normalize_returns=True, **kw)


def test_header_declares_what_the_binding_binds():
    from ddrl4nav_amd import _lib
    text = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    for name in NEW:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [3, 8, 4, 6, 9, 8]
    assert re.search(r"#define\s+DDRL_ABI_VERSION\s+3\b", text) and _lib.ABI_VERSION == 3
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW)
    from ddrl4nav_amd import ops
    assert all(hasattr(ops, n) for n in ("column_moments", "running_merge", "running_affine", "normalize_columns", "discounted_returns"))


def test_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses: every refusal below is decided before the first HIP call."""
    from ctypes import byref, c_int64
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    INVALID = -1
    a, M = 0x10000000, 0x1000000
    f = c_int64()
    ws = lib.ddrl_op_column_moments_ws_floats
    assert ws(0, 1, byref(f)) == INVALID and ws(4, 0, byref(f)) == INVALID and ws(4, 4, None) == INVALID and ws(-1, -1, byref(f)) == INVALID
    assert ws(1, 1, byref(f)) == 0 and f.value == 4                       # one slab of 2 d doubles
    assert ws(131072, 1, byref(f)) == 0 and f.value == 128 * 4           # 1024-row slabs
    assert ws(512, 6912, byref(f)) == 0 and f.value == 32 * 4 * 6912     # 16-row slabs
    assert ws(1 << 40, 960, byref(f)) == 0 and f.value == 256 * 4 * 960  # bounded: a cap on the slabs
    top = (2 ** 63 - 1) // 8                                             # the largest n the operator itself admits
    assert ws(top, 1, byref(f)) == 0 and f.value == 256 * 4 and ws(top, 1 << 28, byref(f)) == 0 and f.value == 256 * 4 << 28
    assert ws(top + 1, 1, byref(f)) == INVALID and ws(2 ** 63 - 1, 1, byref(f)) == INVALID and ws(4, (1 << 28) + 1, byref(f)) == INVALID
    assert lib.ddrl_op_column_moments(a, top + 1, 1, 1, a + M, 0, a + 2 * M, None) == INVALID

    mom = lambda x=a, n=64, d=5, ld=8, s=a + M, ws=a + 2 * M: lib.ddrl_op_column_moments(x, n, d, ld, s, 0, ws, None)
    for kw in (dict(x=None), dict(s=None), dict(ws=None), dict(n=0), dict(n=-3), dict(d=0), dict(d=-1), dict(ld=4), dict(x=a + 2),
               dict(s=a + M + 4), dict(ws=a + 2 * M + 4),
               dict(s=a + 8), dict(s=a + 63 * 32 + 16),                   # the sums inside x's rows, inside its last row
               dict(ws=a + 16), dict(ws=a + M + 8), dict(s=a + 2 * M + 8),  # ws on x, ws on the sums, the sums on ws
               dict(x=a + M - 64 * 32 + 16)):                             # x's last row ends inside the sums
        assert mom(**kw) == INVALID, kw

    mer = lambda s=a, d=5, st=a + M: lib.ddrl_op_running_merge(s, d, st, None)
    for kw in (dict(s=None), dict(st=None), dict(d=0), dict(d=-2), dict(s=a + 4), dict(st=a + M + 4), dict(st=a + 8), dict(st=a + 80),
               dict(st=a - 80)):
        assert mer(**kw) == INVALID, kw

    aff = lambda st=a, d=5, eps=1e-8, out=a + M: lib.ddrl_op_running_affine(st, d, eps, 1, out, None)
    for kw in (dict(st=None), dict(out=None), dict(d=0), dict(st=a + 4), dict(out=a + M + 2), dict(eps=-1.0), dict(eps=float("nan")),
               dict(out=a + 16), dict(out=a + 84), dict(out=a - 36)):
        assert aff(**kw) == INVALID, kw

    def norm(x=a, n=64, d=5, ldx=8, af=a + M, clip=10.0, out=a + 2 * M, ldo=8):
        return lib.ddrl_op_normalize_columns(x, n, d, ldx, af, clip, out, ldo, None)

    for kw in (dict(x=None), dict(af=None), dict(out=None), dict(n=0), dict(d=0), dict(ldx=4), dict(ldo=3), dict(x=a + 1), dict(af=a + M + 2),
               dict(out=a + 2 * M + 3), dict(clip=0.0), dict(clip=-1.0), dict(clip=float("nan")),
               dict(out=a + 4), dict(out=a - 4), dict(out=a + 32),          # shifted by a float, by a row: neither in place nor apart
               dict(out=a, ldo=16), dict(out=a, ldx=16),                    # the same base with other strides
               dict(af=a + 2 * M + 8), dict(af=a + 2 * M - 36),             # the affine inside out, ending inside out
               dict(out=a + 63 * 32 + 16)):                                 # out begins inside x's last row
        assert norm(**kw) == INVALID, kw

    def disc(r=a, dn=a + M, T=4, N=8, gamma=0.99, c=a + 2 * M, tr=a + 3 * M):
        return lib.ddrl_op_discounted_returns(r, dn, T, N, gamma, c, tr, None)

    for kw in (dict(r=None), dict(dn=None), dict(c=None), dict(tr=None), dict(T=0), dict(N=0), dict(N=-4), dict(r=a + 2), dict(c=a + 2 * M + 1),
               dict(tr=a + 3 * M + 2), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")),
               dict(tr=a), dict(tr=a + 124), dict(tr=a + M + 28), dict(tr=a + 2 * M + 28),   # the trace on the rewards, dones, carry
               dict(c=a + 124), dict(c=a + M + 28), dict(c=a + 3 * M + 124)):                # the carry on the rewards, dones, trace
        assert disc(**kw) == INVALID, kw
