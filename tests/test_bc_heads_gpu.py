"""The cloning operators of a Gaussian actor and of fp32 demonstration pools (csrc/imit.hip):
ddrl_op_heads_bc_mse against its float64 statement, and ddrl_op_gather_rows_f32 against numpy indexing.

Stated tolerances (tests/test_generic_cross_gpu.py's): loss and metric rtol 2e-5; dh, dw, db per tensor |d| <= 2e-5 max|want|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FEAT = 512


def mse64(w, b, h, y, n_total):
    """float64: (loss share, sum |mu - y|, dh, dw, db) of mean((mu - y)^2) / 2 over n_total * A elements."""
    w, b, h, y = (np.asarray(a, np.float64) for a in (w, b, h, y))
    d = h @ w.T + b - y
    g = d / (n_total * w.shape[0])
    return (d * d).sum() / (2.0 * n_total * w.shape[0]), np.abs(d).sum(), g @ w, g.T @ h, g.sum(0)


def run_mse(w, b, h, y, n_total, ld):
    from ddrl4nav_amd import ops
    n, A = y.shape
    dev = dict(dtype=torch.float32, device="cuda")
    hd = torch.zeros((n, ld), **dev)
    hd[:, :FEAT] = torch.from_numpy(h)
    guard = float.fromhex("0x1.5p3")
    dh = torch.full((n, ld), guard, **dev)
    arena = torch.from_numpy(np.concatenate([[0.0], w.reshape(-1), b]).astype(np.float32)).cuda()   # the head lies anywhere in an arena
    wd, bd = arena[1:1 + A * FEAT], arena[1 + A * FEAT:]
    grads = torch.full((A * FEAT + A + 2 + 1,), guard, **dev)
    dw, db, stats = grads[1:1 + A * FEAT], grads[1 + A * FEAT:1 + A * FEAT + A], grads[1 + A * FEAT + A:]
    ws = torch.empty(ops.heads_bc_mse_ws_floats(A, n), **dev)
    ops.heads_bc_mse(wd, bd, A, hd, ld, n, torch.from_numpy(y).cuda(), n_total, dh, ld, dw, db, stats, ws)
    assert float(grads[0]) == guard and bool((dh[:, FEAT:] == guard).all())
    return stats.cpu().numpy().astype(np.float64), dh[:, :FEAT].cpu().numpy(), dw.view(A, FEAT).cpu().numpy(), db.cpu().numpy()


@pytest.mark.parametrize("A", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 3, 4, 17, 1030])       # 16 samples per workgroup-turn x 64 workgroups = 1,024: 1,030 wraps the grid
def test_bc_mse_vs_float64(n, A):
    rng = np.random.RandomState(1000 * n + A)
    w = rng.uniform(-0.05, 0.05, (A, FEAT)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, A).astype(np.float32)
    h = np.maximum(rng.normal(0.3, 1.0, (n, FEAT)), 0).astype(np.float32)
    y = rng.normal(0, 1, (n, A)).astype(np.float32)
    for ld, n_total in ((512, n), (520, 2 * n + 3)):
        loss, metric, dh, dw, db = mse64(w, b, h, y, n_total)
        stats, gdh, gdw, gdb = run_mse(w, b, h, y, n_total, ld)
        print("n %d A %d ld %d: loss %.9g (float64 %.9g), sum|d| %.9g (%.9g)" % (n, A, ld, stats[0], loss, stats[1], metric))
        np.testing.assert_allclose(stats, [loss, metric], rtol=2e-5)
        for name, got, want in (("dh", gdh, dh), ("dw", gdw, dw), ("db", gdb, db)):
            err, scale = np.abs(got - want).max(), np.abs(want).max()
            print("   %s: %.2e max|want|" % (name, err / scale))
            assert err <= 2e-5 * scale, (name, n, A, ld, err / scale)
        again = run_mse(w, b, h, y, n_total, ld)
        assert all(np.array_equal(p, q) for p, q in zip((stats, gdh, gdw, gdb), again))     # repeats are bit-identical


# ---- ddrl_op_gather_rows_f32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 300])
@pytest.mark.parametrize("width", [5, 960, 6912])
def test_gather_rows_f32(width, n):
    from ddrl4nav_amd import ops
    rng = np.random.RandomState(width + n)
    n_rows = 41
    src = rng.normal(size=(n_rows, width)).astype(np.float32)
    idx = rng.randint(0, n_rows, n).astype(np.int32)
    idx[0] = idx[-1] = 7                                               # repeated
    if n >= 7:
        idx[1:5] = (-1, n_rows, -2 ** 31, 2 ** 31 - 1)                # outside [0, n_rows): clamped
    want = src[np.clip(idx, 0, n_rows - 1)]
    guard = float.fromhex("0x1.5p3")
    for shift in (0, 1):                                               # 1: a base that is not 16-byte aligned takes the 4-byte path
        store = torch.zeros(n_rows * width + 4, dtype=torch.float32, device="cuda")
        s = store[shift:shift + n_rows * width].view(n_rows, width)
        s.copy_(torch.from_numpy(src))
        out = torch.full(((n + 2) * width + 4,), guard, dtype=torch.float32, device="cuda")
        d = out[shift + width:shift + (n + 1) * width].view(n, width)
        assert (s.data_ptr() % 16 == 0) == (shift == 0)
        ops.gather_rows_f32(s, torch.from_numpy(idx).cuda(), d)
        got = out.cpu().numpy()
        assert np.array_equal(got[shift + width:shift + (n + 1) * width].reshape(n, width), want), (width, n, shift)
        assert (got[:shift + width] == guard).all() and (got[shift + (n + 1) * width:] == guard).all()
