"""GPU tests of the HIP kernels that take their sizes at RUN TIME -- the dense layers (csrc/plin.hip, glinear.hip), the gather
convolutions and the thin weight gradient (csrc/gconv.hip), the run-time width of csrc/c1d.hip and the four max-pool kernels -- at the
edges of their tiles.  The shape tables live in tests/runtime_shapes.py and are built from the kernels' tile constants; every reference
is float64 torch on the CPU from the same fp32 inputs; the tolerance is the operator tolerance of tests/test_ops_gpu.py
(|d| <= 2e-5 max|want| + 1e-7) unless a test says otherwise.

A2 on the parent of the commit that added this module (csrc/plin.hip without the mask in nt_planes_kernel's fetch), on an MI355X: 24 of
the 27 plane-family cases with columns behind K or N failed -- every forward / data-gradient output of a row whose neighbour columns
scaled past fp16's range was NaN (inf x 0 in the matrix pipe); the 3 that passed have K and N that are multiples of 32, so no k-block
reaches behind them.  All 21 f32-family cases, the ws = NULL runs and both weight gradients passed there.  With the mask every case
passes and the A1 outputs are bit-identical to the parent's.  Largest error against float64 as a multiple of the tolerance: A1 0.035,
A2 0.040, A3 0.019, B 0.054 (recorded in tests/golden/margins.json)."""
import functools
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

import runtime_shapes as R

pytestmark = pytest.mark.gpu

TOL = 2e-5
UNSUPPORTED = -2   # DDRL_ERR_UNSUPPORTED
INVALID_ARG = -1   # DDRL_ERR_INVALID_ARG


def close(got, want, tol=TOL, what=""):
    """The close() of tests/test_ops_gpu.py; prints the error as a multiple of the tolerance before it asserts."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(want.abs().max().item(), 1e-30)
    err = (got - want).abs().max().item()
    bound = tol * scale + 1e-7
    print("margin %s %.4f" % (what, err / bound))
    assert err <= bound, (what, err, scale)


def dev(t):
    return t.cuda()


# =========================================================================================================================================
# A. dense operators
# =========================================================================================================================================
DENSE = R.dense_grid()
SENTINEL = -7.25


def test_dense_grid_covers_every_pair_and_both_families():
    assert R.dense_grid_is_pairwise(DENSE)
    assert (1, 1, 4) in {c[:3] for c in DENSE} and (3, 5, 8) in {c[:3] for c in DENSE}
    planes = [R.uses_planes(*c[:3]) for c in DENSE]
    assert any(planes) and not all(planes)


@functools.lru_cache(maxsize=None)
def dense_problem(case):
    """fp32 inputs of one grid case and the float64 results, computed once and shared (never modified)."""
    n, K, N = case[:3]
    g = torch.Generator().manual_seed(1000 * n + 10 * K + N)
    x = torch.randn(n, K, generator=g)
    dz = torch.randn(n, N, generator=g)
    if n > 2:
        x[1] *= 1e-3      # a faint row: hostile columns are sized by the ROW's own maximum
        dz[2] *= 1e-3
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    mask = torch.randn(n, K, generator=g)
    x64, dz64, W64 = x.double(), dz.double(), W.double()
    z = x64 @ W64.t() + b.double()
    din = dz64 @ W64
    want = dict(z=z, relu=z.clamp_min(0), din=din, din_masked=din * (mask > 0), dw=dz64.t() @ x64, db=dz64.sum(0))
    return dict(x=x, dz=dz, W=W, b=b, mask=mask, want=want)


def widen(t, ld, fill):
    """[n][ld] with t in the first columns; the columns behind them hold zeros ("zeros"), finite values 1e4 x the row's own largest
    magnitude with alternating signs ("neighbour": the next slice of a torch.cat buffer), or +-3e38 ("huge")."""
    n, width = t.shape
    full = torch.zeros(n, ld)
    full[:, :width] = t
    if ld > width and fill != "zeros":
        sign = torch.tensor([1.0, -1.0]).repeat((ld - width + 1) // 2)[:ld - width]
        if fill == "huge":
            full[:, width:] = 3e38 * sign
        else:
            amax = t.abs().amax(1, keepdim=True)
            full[:, width:] = 1e4 * torch.where(amax > 0, amax, torch.ones_like(amax)) * sign
    return full


def widen_mask(mask, ld, fill):
    full = torch.zeros(mask.shape[0], ld)
    full[:, :mask.shape[1]] = mask
    if ld > mask.shape[1] and fill != "zeros":   # non-positive and large values behind K
        pat = torch.tensor([-1.0, 1e30, 0.0, -1e30]).repeat((ld - mask.shape[1] + 3) // 4)
        full[:, mask.shape[1]:] = pat[:ld - mask.shape[1]]
    return full


@functools.lru_cache(maxsize=None)
def dense_layer(K, N, max_n):
    from ddrl4nav_amd.ops import Linear
    return Linear(K, N, max_n=max_n)


def run_dense(case, fill, how):
    """All five launches of one grid case.  how: "wrapper" (the Linear class of ddrl4nav_amd/ops.py), "abi" (the C ABI directly, with
    the layer's workspace), "nows" (the C ABI with ws = NULL: forward and data gradient on the f32-input kernels, no weight gradient).
    Every output lies in a sentinel-filled buffer wider than the result; returns the whole buffers on the CPU."""
    from ddrl4nav_amd import _lib
    from ddrl4nav_amd.ops import _p, _st
    n, K, N, ld_in, ld_dout, ld_out = case
    p = dense_problem(case)
    lin = dense_layer(K, N, 257)
    lin.pack(dev(p["W"]))
    ld_din, ld_mask = R.round_up(K, 4) + 4, ld_in + 4
    xd, dzd, bd = dev(widen(p["x"], ld_in, fill)), dev(widen(p["dz"], ld_dout, fill)), dev(p["b"])
    md = dev(widen_mask(p["mask"], ld_mask, fill))
    new = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    out_relu, out, din, din_masked = new(n, ld_out), new(n, ld_out), new(n, ld_din), new(n, ld_din)
    dwbuf = new(64 + N * K + 64 + N + 64)
    dw, db = dwbuf[64:64 + N * K].view(N, K), dwbuf[128 + N * K:128 + N * K + N]
    lib = lin.lib
    if how == "wrapper":
        lin.forward(xd, ld_in, bd, True, out_relu, ld_out, n)
        lin.forward(xd, ld_in, bd, False, out, ld_out, n)
        lin.dgrad(dzd, ld_dout, None, 0, din, ld_din, n)
        lin.dgrad(dzd, ld_dout, md, ld_mask, din_masked, ld_din, n)
        lin.wgrad(xd, ld_in, dzd, ld_dout, dw, db, n)
    else:
        ws = _p(lin.ws) if how == "abi" else None
        for act, o in ((1, out_relu), (0, out)):
            _lib.check(lib.ddrl_op_linear_forward(_p(xd), ld_in, _p(lin.wt), _p(bd), act, _p(o), ld_out, n, K, N, ws, None, _st()))
        for m, ldm, o in ((None, 0, din), (_p(md), ld_mask, din_masked)):
            _lib.check(lib.ddrl_op_linear_dgrad(_p(dzd), ld_dout, _p(lin.wn), m, ldm, _p(o), ld_din, n, K, N, ws, None, None, 0, 0, _st()))
        status = lib.ddrl_op_linear_wgrad(_p(xd), ld_in, _p(dzd), ld_dout, ws, _p(dw), _p(db), n, K, N, None, None, _st())
        assert status == (0 if how == "abi" else INVALID_ARG)   # the weight gradient has no arm without a workspace
    torch.cuda.synchronize()
    return dict(relu=out_relu.cpu(), z=out.cpu(), din=din.cpu(), din_masked=din_masked.cpu(), dwbuf=dwbuf.cpu(), has_wgrad=how != "nows")


def check_dense(case, res, tag):
    """Results against float64, and every float outside the results still the sentinel."""
    n, K, N = case[:3]
    want = dense_problem(case)["want"]
    for key, width in (("relu", N), ("z", N), ("din", K), ("din_masked", K)):
        assert bool(torch.isfinite(res[key][:, :width]).all()), (tag, key)
        close(res[key][:, :width], want[key], what="A %s %s %s" % (tag, key, case[:3]))
        assert bool((res[key][:, width:] == SENTINEL).all()), (tag, key, "wrote past the result")
    buf = res["dwbuf"]
    dw, db = buf[64:64 + N * K].view(N, K), buf[128 + N * K:128 + N * K + N]
    outside = torch.cat([buf[:64], buf[64 + N * K:128 + N * K], buf[128 + N * K + N:]])
    assert bool((outside == SENTINEL).all()), (tag, "weight gradient wrote past dw / db")
    if res["has_wgrad"]:
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), tag
        close(dw, want["dw"], what="A %s dw %s" % (tag, case[:3]))
        close(db, want["db"], what="A %s db %s" % (tag, case[:3]))
    else:
        assert bool((buf == SENTINEL).all())


def same_bits(a, b, tag):
    for key in ("relu", "z", "din", "din_masked", "dwbuf"):
        assert torch.equal(a[key], b[key]), (tag, key)


@pytest.mark.parametrize("case", DENSE, ids=lambda c: "n%d-K%d-N%d" % c[:3])
def test_dense_boundary_grid_vs_float64(case):
    """A1: forward with / without ReLU, data gradient with / without mask_src, weight and bias gradient through the Linear wrapper, in
    leading dimensions wider than the results; the family each case runs on is the one its sizes say."""
    n, K, N = case[:3]
    assert dense_layer(K, N, 257).uses_planes(n) == R.uses_planes(n, K, N)
    check_dense(case, run_dense(case, "zeros", "wrapper"), "wrapper")


HOSTILE = [c for c in DENSE if c[3] > c[1] or c[4] > c[2]]
# the one plane case and the one f32 case that also run with +-3e38 behind their columns
HUGE = {next(c for c in HOSTILE if R.uses_planes(*c[:3]) and c[1] % 32 and c[2] % 32 and c[3] > c[1] and c[4] > c[2]),
        next(c for c in HOSTILE if not R.uses_planes(*c[:3]) and c[0] > 1 and c[3] > c[1] and c[4] > c[2])}


@pytest.mark.parametrize("case", HOSTILE, ids=lambda c: "n%d-K%d-N%d-ldin%d-lddout%d" % c[:5])
def test_dense_columns_behind_K_and_N_do_not_reach_the_result(case):
    """A2: the columns [K, ld_in) of `in` and [N, ld_dout) of `dout` (and what lies behind K in a wide mask_src) belong to the caller --
    padding, or the neighbouring slice of a torch.cat buffer.  With finite values 1e4 x the row's own maximum there (3e38 in two cases)
    every result is bit-identical to the run with zeros there, finite, and right against float64: through the C ABI with the
    workspace (plane kernels from 128 rows on, f32-input kernels below) and with ws = NULL (f32-input kernels at every size)."""
    assert any(R.uses_planes(*c[:3]) for c in HOSTILE) and any(not R.uses_planes(*c[:3]) for c in HOSTILE)
    for how in ("abi", "nows"):
        zeros = run_dense(case, "zeros", how)
        for fill in ("neighbour", "huge") if case in HUGE else ("neighbour",):
            hostile = run_dense(case, fill, how)
            check_dense(case, hostile, how + "-" + fill)
            same_bits(hostile, zeros, (how, fill))
        check_dense(case, zeros, how + "-zeros")


def test_dense_huge_cases_exist_on_both_families():
    assert len(HUGE) == 2 and {R.uses_planes(*c[:3]) for c in HUGE} == {True, False}


# ---- A3: caller-supplied row magnitudes ------------------------------------------------------------------------------------------------
# plane launches (n >= 128) at K, N of the grid: (n, K, N, ld_in, ld_dout)
AMAX_CASES = [
    (128, 129, 68, 172, 72),     # one row tile; K and N inside a k-block, hostile columns behind both
    (257, 161, 132, 164, 172),   # three row tiles, two column tiles
    (129, 257, 260, 260, 260),   # three column tiles both ways, dense dout
]


def amax_problem(case, rows="plain"):
    n, K, N, ld_in, ld_dout = case
    g = torch.Generator().manual_seed(n + K + N)
    x, dz = torch.randn(n, K, generator=g), torch.randn(n, N, generator=g)
    if rows == "mixed":
        x[3], dz[3] = 0.0, 0.0         # a zero row, magnitude 0
        x[5] *= 1e-5                   # rows 1e-5 below the others
        dz[6] *= 1e-5
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.zeros(N) if rows == "mixed" else torch.randn(N, generator=g)
    return x, dz, W, b


def run_with_magnitudes(case, x, dz, W, b, in_amax, dout_amax):
    """forward, data gradient, weight gradient of a plane launch with the given magnitude arrays (None: the operators' own pre-pass)."""
    n, K, N, ld_in, ld_dout = case
    lin = dense_layer(K, N, 257)
    assert lin.uses_planes(n)
    lin.pack(dev(W))
    xd, dzd, bd = dev(widen(x, ld_in, "neighbour")), dev(widen(dz, ld_dout, "neighbour")), dev(b)
    out, din = torch.empty(n, N, device="cuda"), torch.empty(n, K, device="cuda")
    dw, db = torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda")
    lin.forward(xd, ld_in, bd, False, out, N, n, in_amax=in_amax)
    lin.dgrad(dzd, ld_dout, None, 0, din, K, n, dout_amax=dout_amax)
    lin.wgrad(xd, ld_in, dzd, ld_dout, dw, db, n, in_amax=in_amax, dout_amax=dout_amax)
    return out.cpu(), din.cpu(), dw.cpu(), db.cpu()


def exact_magnitudes(case, x, dz):
    n, K, N, ld_in, ld_dout = case
    lin = dense_layer(K, N, 257)
    a = lin.row_amax(dev(widen(x, ld_in, "neighbour")), ld_in, K, n, torch.empty(n, device="cuda"))
    d = lin.row_amax(dev(widen(dz, ld_dout, "neighbour")), ld_dout, N, n, torch.empty(n, device="cuda"))
    assert torch.equal(a.cpu(), x.abs().amax(1)) and torch.equal(d.cpu(), dz.abs().amax(1))
    return a, d


@pytest.mark.parametrize("case", AMAX_CASES)
def test_dense_exact_magnitudes_equal_the_prepass_bit_for_bit(case):
    x, dz, W, b = amax_problem(case)
    a, d = exact_magnitudes(case, x, dz)
    own = run_with_magnitudes(case, x, dz, W, b, None, None)
    given = run_with_magnitudes(case, x, dz, W, b, a, d)
    for got, ref, name in zip(given, own, ("forward", "dgrad", "dw", "db")):
        assert torch.equal(got, ref), name


@pytest.mark.parametrize("factor", [1.5, 2.0, 1024.0])
@pytest.mark.parametrize("case", AMAX_CASES)
def test_dense_upper_bound_magnitudes_stay_within_tolerance(case, factor):
    """Any upper bound is valid (include/ddrl.h).  x 1.5 crosses a binade for some rows only, x 2 for all, x 2^10 moves every row ten
    binades down: with the maximum mapped to [2^12, 2^13) elements down to 2^-16 of it keep 22 bits (csrc/engine2.h), so a bound 2^10
    too large still keeps them down to 2^-6 of the maximum and loses at most 2^-25 / S = 2^-27 of the maximum (absolute) below that."""
    x, dz, W, b = amax_problem(case)
    a, d = exact_magnitudes(case, x, dz)
    out, din, dw, db = run_with_magnitudes(case, x, dz, W, b, a * factor, d * factor)
    x64, dz64, W64 = x.double(), dz.double(), W.double()
    tag = "A3 x%g %s " % (factor, case[:3])
    close(out, x64 @ W64.t() + b.double(), what=tag + "forward")
    close(din, dz64 @ W64, what=tag + "dgrad")
    close(dw, dz64.t() @ x64, what=tag + "dw")
    close(db, dz64.sum(0), what=tag + "db")


@pytest.mark.parametrize("case", AMAX_CASES)
def test_dense_given_magnitudes_keep_rows_of_mixed_size(case):
    """A zero row with magnitude 0 and rows 1e-5 below the others, each with its own exact magnitude: per-row accuracy as in
    test_linear_rows_of_very_different_magnitude_keep_their_precision (2e-6 of the row's own largest result)."""
    x, dz, W, b = amax_problem(case, rows="mixed")
    a, d = exact_magnitudes(case, x, dz)
    assert float(a[3]) == 0.0 and float(d[3]) == 0.0
    out, din, dw, db = run_with_magnitudes(case, x, dz, W, b, a, d)
    x64, dz64, W64 = x.double(), dz.double(), W.double()
    for got, want in ((out, x64 @ W64.t()), (din, dz64 @ W64)):
        row = want.abs().amax(1, keepdim=True).clamp_min(1e-300)
        assert float(((got.double() - want).abs() / row).max()) < 2e-6
        assert float(got[3].abs().max()) == 0.0
    close(dw, dz64.t() @ x64, what="A3 mixed dw %s" % (case[:3],))
    close(db, dz64.sum(0), what="A3 mixed db %s" % (case[:3],))


@pytest.mark.parametrize("width", [1, 3, 4, 5, 255, 256, 257])   # around one 4-float load and around one 256-float pass of a wave
def test_row_amax_reads_its_columns_only(width):
    """ddrl_op_row_amax inside rows whose remaining columns are hostile; accumulate = 1 raises a zeroed array to the same values and
    never lowers a pre-raised slot."""
    lin = dense_layer(128, 64, 257)
    n, ld = 9, R.round_up(width, 4) + 8
    g = torch.Generator().manual_seed(width)
    x = torch.randn(n, width, generator=g)
    x[2] = 0.0
    x[4] *= 1e-6
    full = widen(x, ld, "neighbour")
    full[2, width:] = 5.0
    want = x.abs().amax(1)
    xd = dev(full)
    assert torch.equal(lin.row_amax(xd, ld, width, n, torch.full((n,), -1.0, device="cuda")).cpu(), want)
    assert torch.equal(lin.row_amax(xd, ld, width, n, torch.zeros(n, device="cuda"), accumulate=True).cpu(), want)
    raised = torch.zeros(n)
    raised[1], raised[2] = 1e30, 1e-30
    got = lin.row_amax(xd, ld, width, n, dev(raised), accumulate=True).cpu()
    assert torch.equal(got, torch.maximum(want, raised))


@pytest.mark.parametrize("case", [c for c in DENSE if c[1] >= 128][::3], ids=lambda c: "n%d-K%d-N%d" % c[:3])
def test_dense_data_gradient_magnitudes_over_column_ranges(case):
    """din_amax over ranges that start and end inside a 128-column tile and that end at K (also where K is no multiple of 4): exactly
    the maximum over what was written, masked elements counting as zeros; both families."""
    n, K, N, ld_in, ld_dout, _ = case
    p = dense_problem(case)
    lin = dense_layer(K, N, 257)
    lin.pack(dev(p["W"]))
    ld_din = R.round_up(K, 4) + 4
    dzd, md = dev(widen(p["dz"], ld_dout, "neighbour")), dev(widen_mask(p["mask"], ld_in, "neighbour"))
    for lo, hi in R.amax_ranges(K):
        for mask in (None, md):
            din = torch.full((n, ld_din), SENTINEL, device="cuda")
            amax = torch.zeros(n, device="cuda")
            lin.dgrad(dzd, ld_dout, mask, ld_in if mask is not None else 0, din, ld_din, n, din_amax=amax, amax_cols=(lo, hi))
            assert torch.equal(amax, din[:, lo:hi].abs().amax(1)), (lo, hi, mask is not None)
            assert bool((din[:, K:] == SENTINEL).all())


# =========================================================================================================================================
# B. gather convolutions, thin weight gradient, the run-time width of c1d.hip
# =========================================================================================================================================
def reached_inputs(shape):
    """[h][w] bool: input positions that at least one tap of one output reads."""
    n, cin, h, w, cout, kh, kw, s, pad = shape
    probe = torch.zeros(1, 1, h, w, dtype=torch.float64, requires_grad=True)
    F.conv2d(probe, torch.ones(1, 1, kh, kw, dtype=torch.float64), stride=s, padding=pad).sum().backward()
    return probe.grad[0, 0] > 0


def check_conv(shape, xin=0, xout=0, family="gather", seed=0):
    """Forward with / without ReLU, data gradient, weight + bias gradient of one layer through the C ABI against float64 autograd,
    on sample records `xin` / `xout` floats wider than dense with sentinels between the samples of every written tensor."""
    from ddrl4nav_amd import _lib
    from ddrl4nav_amd.ops import Conv, _p, _st
    n, cin, h, w, cout, kh, kw, s, pad = shape
    conv = Conv(cin, h, w, cout, kh, kw, stride=s, pad=pad, max_n=n)
    oh, ow = R.conv_out(h, w, kh, kw, s, pad)
    assert (conv.oh, conv.ow) == (oh, ow)
    # no specialised family takes the shape: no plane scratch, no pooling epilogue, outside the tables of planes_id / first_id / c1d_id
    assert conv.scratch is None and not conv.has_forward_pool()
    assert R.conv_is_c1d(shape) == (family == "c1d") and not R.conv_is_first(shape) and not R.conv_is_planes(shape)
    ein, eout = cin * h * w, cout * oh * ow
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, ein + xin, generator=g)
    wt = torch.randn(cout, cin, kh, kw, generator=g) / (cin * kh * kw) ** 0.5
    b = torch.randn(cout, generator=g)
    dz = torch.randn(n, eout + xout, generator=g)
    x64 = x[:, :ein].reshape(n, cin, h, w).double().requires_grad_(True)
    wt64, b64 = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    z = F.conv2d(x64, wt64, b64, stride=s, padding=pad)
    z.backward(dz[:, :eout].reshape(z.shape).double())
    conv.pack(dev(wt))
    lib = conv.lib
    d = conv.desc(n, in_sn=ein + xin if xin else 0, out_sn=eout + xout if xout else 0)
    xd, bd, dzd = dev(x), dev(b), dev(dz)
    tag = "B %s" % (shape,)
    for act, want in ((1, z.detach().clamp_min(0)), (0, z.detach())):
        out = torch.full((n, eout + xout), SENTINEL, device="cuda")
        _lib.check(lib.ddrl_op_conv_forward(byref(d), _p(xd), _p(conv.packed), _p(bd), act, _p(out), None, None, _st()))
        close(out[:, :eout].reshape(z.shape), want, what=tag + " forward act=%d" % act)
        assert bool((out[:, eout:] == SENTINEL).all())
    got = out[:, :eout].reshape(z.shape).cpu()
    if pad[0] >= kh:   # padding at least the kernel size: the outermost outputs see zeros only and equal the bias
        assert torch.equal(got[:, :, 0, :], b[None, :, None].expand(n, cout, ow))
    if pad[1] >= kw:
        assert torch.equal(got[:, :, :, 0], b[None, :, None].expand(n, cout, oh))
    din = torch.full((n, ein + xin), SENTINEL, device="cuda")
    _lib.check(lib.ddrl_op_conv_dgrad(byref(d), _p(dzd), _p(conv.packed), _p(din), None, _st()))
    din_c = din[:, :ein].reshape(n, cin, h, w).cpu()
    close(din_c, x64.grad, what=tag + " dgrad")
    assert bool((din[:, ein:] == SENTINEL).all())
    unread = ~reached_inputs(shape)
    assert int(unread.sum()) == 0 or float(din_c[:, :, unread].abs().max()) == 0.0   # exactly 0 where no tap reaches
    dwbuf = torch.full((64 + wt.numel() + 64 + cout + 64,), SENTINEL, device="cuda")
    dw, db = dwbuf[64:64 + wt.numel()], dwbuf[128 + wt.numel():128 + wt.numel() + cout]
    status = lib.ddrl_op_conv_wgrad(byref(d), _p(xd), _p(dzd), _p(conv.packed), _p(conv.ws), _p(dw), _p(db), _st())
    torch.cuda.synchronize()
    if oh * ow >= 32:
        assert status == 0
        close(dw.view(wt.shape), wt64.grad, what=tag + " dw")
        close(db, b64.grad, what=tag + " db")
        dwbuf[64:64 + wt.numel()] = SENTINEL
        dwbuf[128 + wt.numel():128 + wt.numel() + cout] = SENTINEL
    else:
        assert status == UNSUPPORTED
    assert bool((dwbuf == SENTINEL).all())   # nothing outside dw / db (oh ow < 32: nothing at all)


def test_conv_table_claims():
    """What the comments of the geometry table promise about k-blocks and splits, from the mirrors of the host-side arithmetic."""
    by_cols = {s[0] * R.conv_out(*s[2:4], *s[5:9])[0] * R.conv_out(*s[2:4], *s[5:9])[1] for s in R.CONV_GEOMETRIES}
    assert {255, 256, 257} <= by_cols
    assert {1, 63, 64, 65} <= {s[4] for s in R.CONV_GEOMETRIES}
    assert {15, 16, 17, 33} <= {s[1] * s[5] * s[6] for s in R.CONV_GEOMETRIES}
    planes = {R.conv_out(*s[2:4], *s[5:9])[0] * R.conv_out(*s[2:4], *s[5:9])[1] for s in R.CONV_GEOMETRIES}
    assert {32, 33, 35, 47} <= planes
    lens = [[e - b for b, e in R.conv_wgrad_split_ranges(s)] for s in R.CONV_GEOMETRIES]
    assert any(len(l) > 1 and 0 < l[-1] < l[0] for l in lens)      # an uneven last split
    assert any(l[-1] == 0 and l[0] > 0 for l in lens)              # empty splits
    assert all(not R.conv_is_specialised(s) for s in R.CONV_GEOMETRIES + R.CONV_SMALL_PLANES)


@pytest.mark.parametrize("shape", R.CONV_GEOMETRIES)
def test_gather_conv_geometry_table_vs_float64(shape):
    check_conv(shape, seed=R.CONV_GEOMETRIES.index(shape))


@pytest.mark.parametrize("n_w", R.C1D_WIDTHS)
def test_conv1d_runtime_width_vs_float64(n_w):
    """The one specialised item: Conv1d(32, 32, 3, stride 2) of csrc/c1d.hip at output lengths around the 64 positions a wave of its
    weight gradient takes per chunk."""
    shape = R.c1d_shape(*n_w)
    assert R.conv_out(1, n_w[1], 1, 3, 2, (0, 0))[1] in (R.C1D_CHUNK - 1, R.C1D_CHUNK, R.C1D_CHUNK + 1, 2 * R.C1D_CHUNK + 1)
    check_conv(shape, family="c1d", seed=n_w[1])


@pytest.mark.parametrize("item", R.CONV_STRIDED)
def test_gather_conv_in_strided_sample_records(item):
    """B2: in_sn / out_sn wider than dense by amounts that are no multiples of 4 floats; the reference sees the dense slices."""
    index, xin, xout = item
    shape = R.CONV_GEOMETRIES[index]
    n, cin, h, w, cout, kh, kw, s, pad = shape
    oh, ow = R.conv_out(h, w, kh, kw, s, pad)
    assert (cin * h * w + xin) % 4 and (cout * oh * ow + xout) % 4
    check_conv(shape, xin=xin, xout=xout, seed=100 + index)


@pytest.mark.parametrize("shape", R.CONV_SMALL_PLANES)
def test_conv_weight_gradient_needs_32_outputs_per_plane(shape):
    """B3: oh ow < 32 -- ddrl_op_conv_wgrad answers DDRL_ERR_UNSUPPORTED and writes nothing; forward and data gradient of the same
    layer work (check_conv keeps sentinels in and around dw / db and asserts the status by oh ow)."""
    check_conv(shape, seed=200 + shape[0])


@pytest.mark.parametrize("t", R.THIN + R.NOT_THIN)
def test_thin_weight_gradient_every_tap_count(t):
    """B4: thin_wgrad_kernel<1..6> (KT = cin kw), cout 1 / 5 / 32, strides 1 / 2 / 4, padded and not, one sample, a few, and more than
    THIN_WGS; the two shapes just outside (KT = 7, cout = 33) take the MFMA weight gradient and must give the same answer."""
    shape = R.thin_shape(t)
    n, cin, w, cout, kw, s, pw = t
    assert R.conv_is_thin(shape) == (t in R.THIN)
    assert R.conv_out(1, w, 1, kw, s, (0, pw))[1] >= 32
    check_conv(shape, seed=300 + (R.THIN + R.NOT_THIN).index(t))


def test_thin_table_claims():
    assert {t[1] * t[4] for t in R.THIN} == {1, 2, 3, 4, 5, 6}
    assert {(2, 3), (3, 2)} <= {(t[1], t[4]) for t in R.THIN}
    assert {t[3] for t in R.THIN} == {1, 5, 32} and {t[5] for t in R.THIN} == {1, 2, 4} and {t[6] for t in R.THIN} == {0, 2}
    assert {t[0] for t in R.THIN} == {1, 7, 515} and 515 > R.THIN_WGS
    assert {(t[1] * t[4], t[3]) for t in R.NOT_THIN} == {(7, 32), (6, 33)}


# =========================================================================================================================================
# C. max-pool kernels
# =========================================================================================================================================
def pool_input(planes_hw):
    (n, c), h, w = planes_hw
    g = torch.Generator().manual_seed(h * 100 + w)
    z = torch.randn(n, c, h, w, generator=g)
    # the first windows of plane (0, 0), row-major: an exact tie of the maximum in every pair of window positions, then a window that
    # is negative throughout, then one whose maximum is exactly 0
    windows = [[1.5 if k in (i, j) else -0.5 - k for k in range(4)] for i in range(4) for j in range(i + 1, 4)]
    windows += [[-1.0, -2.0, -0.5, -3.0], [-1.0, 0.0, -2.0, 0.0]]
    flat = z[0, 0].reshape(h // 2, 2, w // 2, 2).permute(0, 2, 1, 3).reshape(-1, 4)
    count = min(len(windows), flat.shape[0])
    flat[:count] = torch.tensor(windows[:count])
    z[0, 0] = flat.reshape(h // 2, w // 2, 2, 2).permute(0, 2, 1, 3).reshape(h, w)
    return z, g


@pytest.mark.parametrize("planes_hw", R.POOLS)
def test_maxpool_kernels_bit_exact_vs_torch_autograd(planes_hw):
    from ddrl4nav_amd.ops import maxpool2, maxpool2_relu_backward, maxpool2_idx, maxpool2_backward_idx
    (n, c), h, w = planes_hw
    z, g = pool_input(planes_hw)
    z.requires_grad_(True)
    a = F.relu(z)
    pooled = F.max_pool2d(a, 2, stride=2)
    dpool = torch.randn(pooled.shape, generator=g)
    pooled.backward(dpool)
    ad, zd, dpd = dev(a.detach()), dev(z.detach()), dev(dpool)
    assert torch.equal(maxpool2(ad).cpu(), pooled.detach())
    assert torch.equal(maxpool2(zd).cpu(), F.max_pool2d(z.detach(), 2, stride=2))      # negative maxima too
    assert torch.equal(maxpool2_relu_backward(ad, dpd).cpu(), z.grad)
    out, code = maxpool2_idx(ad)
    assert torch.equal(out.cpu(), pooled.detach()) and int(code.max()) < 8
    dz = maxpool2_backward_idx(dpd, code, h, w)
    assert torch.equal(dz.cpu(), z.grad)
    # from the pre-activation itself: same first maximum wherever it is positive, no gradient elsewhere
    out_z, code_z = maxpool2_idx(zd)
    assert torch.equal(out_z.cpu(), F.max_pool2d(z.detach(), 2, stride=2))
    assert torch.equal(maxpool2_backward_idx(dpd, code_z, h, w).cpu(), z.grad)
    # views the pair kernel (W % 4 == 0) cannot load: d(pooled) 4- but not 8-byte aligned, decision bytes at an odd address -- the quad
    # kernel serves them (it serves W % 4 == 2 anyway) and gives the aligned run's bits
    numel = dpool.numel()
    dp_odd = torch.zeros(numel + 3, device="cuda")[1:1 + numel].view(dpool.shape)
    dp_odd.copy_(dpd)
    code_odd = torch.zeros(numel + 3, dtype=torch.uint8, device="cuda")[1:1 + numel].view(code.shape)
    code_odd.copy_(code)
    assert dp_odd.data_ptr() % 8 == 4 and code_odd.data_ptr() % 2 == 1
    for dp_v, code_v in ((dp_odd, code), (dpd, code_odd), (dp_odd, code_odd)):
        assert torch.equal(maxpool2_backward_idx(dp_v, code_v, h, w), dz)


def test_pool_table_claims():
    per_wg = R.POOL_QUADS * R.POOL_THREADS
    quads = {(w % 4, n * c * h * w // 4) for (n, c), h, w in R.POOLS}
    assert any(m == 2 and q > per_wg and q % per_wg for m, q in quads) and any(m == 2 and q < per_wg for m, q in quads)
    assert any(m == 0 and q // 2 > per_wg and (q // 2) % per_wg for m, q in quads) and any(m == 0 and q // 2 < per_wg for m, q in quads)
