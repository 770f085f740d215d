"""Imitation pre-training (nn/imitation.py, csrc/imit.hip) on the GPU: the cross-entropy head and the minibatch gather through
the C ABI, and ``net.imitation_learning`` end to end.  Run with `-m gpu`.

Yardstick: torch in float64, built inline (the reference cannot run this path: its ``criterion(self(X), Y)`` fails on a PPO net).
The loss kernel is judged as tests/test_heads_optim_ops_gpu.py judges the PPO loss block -- its mean error against float64 beside
torch's own fp32 (CPU) evaluation of the same expression on the same inputs, err_kernel <= VS_TORCH_LIMIT x err_torch32, the raw
ratio logged through P.MARGINS; a yardstick below the rounding floor or a mean over fewer than 64 draws has no ratio and takes the
operator tolerance 2e-5 (judge()).  Errors are relative to the tensor's largest float64 magnitude, those of d(features) row by
row to the row's; the draws behind d(features) are the rows that carry a gradient (a row whose softmax is one-hot to rounding
has none).

Three optimiser steps: per parameter tensor, L2 deviation of the kernels' parameters from the float64 run over the same deviation
of a torch-fp32 run on the same batches, limit 2.0 (tests/golden/margins.json records up to 1.74 for ten PPO steps through the same
encoder kernels against a single fp32 implementation, and DESIGN.md documents the plane scheme's 22-bit floor)."""
import types
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity_util as P

pytestmark = pytest.mark.gpu

SENT = 7.25
OP_TOL = 2e-5            # tests/test_ops_gpu.py close(): same products, other summation order
FLOOR = 2.0 ** -25       # mean relative error of a correctly rounded fp32 tensor: no yardstick below it
MIN_DRAWS = 64
STEP_LIMIT = 2.0
FEAT = 512
INVALID, UNSUPPORTED = -1, -2


def _p(t):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def _st():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from ddrl4nav_amd import _lib
    return _lib, _lib.load()


def judge(key, err_k, err_32, draws, where):
    """err_kernel <= 1.25 x err_torch32 on the raw ratio of the two mean errors (both relative to the quantity's scale).  No ratio
    -- the operator tolerance instead -- when the yardstick is below the rounding floor (torch's result is correctly rounded, the
    ratio is noise) or fewer than MIN_DRAWS independent draws stand behind the means (the ratio of two means of k draws of |noise|
    scatters by about 1.06 / sqrt(k): 0.13 at k = 64 against a margin of 0.25)."""
    err_k, err_32 = float(err_k), float(err_32)
    ratio = err_k / err_32 if err_32 > 0 else float("inf")
    print("%-24s kernel %.3e  torch32 %.3e  ratio %-8.3f draws %-6d %s" % (key, err_k, err_32, ratio, draws, where))
    if err_32 > FLOOR and draws >= MIN_DRAWS:
        P.MARGINS.check("accuracy", key + "_vs_torch_fp32", ratio, "(%s: kernel %.3e, torch fp32 %.3e)" % (where, err_k, err_32))
    else:
        assert err_k <= OP_TOL, (key, where, err_k, err_32)


# ---- 1. the loss kernel ------------------------------------------------------------------------------------------------------------
def bc_inputs(A, n, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(1000 * A + n + seed)
    h = torch.randn((n, FEAT), generator=g)
    w = torch.randn((A, FEAT), generator=g) * (2.0 * scale / FEAT ** 0.5)
    b = torch.randn((A,), generator=g) * 0.1
    y = torch.randint(0, A, (n,), generator=g).float()
    y[0], y[-1] = 0.0, float(A - 1)
    return h, w, b, y


def bc_torch(h, w, b, y, n_total, dtype):
    h = h.to(dtype).requires_grad_(True)
    w = w.to(dtype).requires_grad_(True)
    b = b.to(dtype).requires_grad_(True)
    z = h @ w.t() + b
    loss = F.cross_entropy(z, y.long(), reduction="sum") / n_total
    loss.backward()
    return {"loss": loss.detach().double(), "dh": h.grad.double(), "dw": w.grad.double(), "db": b.grad.double(),
            "correct": int((z.argmax(1) == y.long()).sum()), "z": z.detach().double()}


def run_bc(h, w, b, y, n_total, ld_h=512, ld_dh=512):
    """The kernel on h placed in rows of ld_h floats, w / b at odd offsets of a parameter arena, dw / db at the same offsets of a
    gradient arena; everything around the outputs is checked to be untouched."""
    _l, lib = _lib()
    n, A = h.shape[0], w.shape[0]
    f = dict(dtype=torch.float32, device="cuda")
    wo, bo, so = 3, 3 + A * FEAT + 2, 3 + A * FEAT + 2 + A + 1       # 4-byte aligned only
    total = so + 2 + 5
    params = torch.full((total,), 0.5, **f)
    params[wo:wo + A * FEAT] = w.reshape(-1).cuda()
    params[bo:bo + A] = b.cuda()
    grads = torch.full((total,), SENT, **f)
    hbuf = torch.full((n, ld_h), 0.25, **f)
    hbuf[:, :FEAT] = h.cuda()
    dh = torch.full((n + 2, ld_dh), SENT, **f)
    wf = c_int64()
    _l.check(lib.ddrl_op_heads_bc_ws_floats(A, n, byref(wf)))
    ws = torch.zeros(wf.value, **f)
    yd = y.cuda()
    _l.check(lib.ddrl_op_heads_bc_loss(_p(params[wo:]), _p(params[bo:]), A, _p(hbuf), ld_h, n, _p(yd), n_total, _p(dh), ld_dh,
                                       _p(grads[wo:]), _p(grads[bo:]), _p(grads[so:]), _p(ws), _st()))
    torch.cuda.synchronize()
    g, d = grads.cpu(), dh.cpu()
    mask = torch.ones(total, dtype=torch.bool)
    for o, c in ((wo, A * FEAT), (bo, A), (so, 2)):
        mask[o:o + c] = False
    assert bool((g[mask] == SENT).all()), "gradient arena written outside dw / db / stats"
    assert bool((d[n:] == SENT).all()) and bool((d[:, FEAT:] == SENT).all()), "dh written outside [n][512]"
    return {"loss": g[so].double(), "correct": float(g[so + 1]), "dh": d[:n, :FEAT].double(),
            "dw": g[wo:wo + A * FEAT].reshape(A, FEAT).double(), "db": g[bo:bo + A].double()}


def check_bc(got, r64, r32, n, where, key="bc"):
    assert got["correct"] == r64["correct"], (where, got["correct"], r64["correct"])
    for name in ("loss", "dh", "dw", "db"):
        k, w, t = got[name], r64[name], r32[name]
        assert bool(torch.isfinite(k).all()), (name, where)
        scale = max(float(w.abs().max()), 1e-300)
        assert float((k - w).abs().max()) <= OP_TOL * scale + 1e-7, (name, where, float((k - w).abs().max()), scale)
        if name == "dh":       # row by row, each relative to its own largest magnitude; the draws are the rows with a gradient
            rowmax = w.abs().amax(1)
            rows = rowmax > 1e-4 * scale
            draws = int(rows.sum())
            ek, et = ((k - w).abs().amax(1) / rowmax)[rows].mean(), ((t - w).abs().amax(1) / rowmax)[rows].mean()
        else:
            draws = {"loss": 1, "dw": n, "db": w.numel()}[name]
            ek, et = (k - w).abs().mean() / scale, (t - w).abs().mean() / scale
        judge("%s_%s" % (key, name), ek, et, draws, where)


BC_A = (2, 6, 7, 8, 9, 18)      # every template boundary of the head kernels (6 / 8 / 18)
BC_N = (1, 3, 5, 63, 257)       # below, at and across a wave's samples per turn (4) and a workgroup's share (16)


@pytest.mark.parametrize("n", BC_N)
@pytest.mark.parametrize("A", BC_A)
def test_bc_loss_vs_float64(A, n):
    i = BC_A.index(A) + BC_N.index(n)
    ld_h, ld_dh = (528, 512) if i % 2 else (512, 528)
    n_total = 3 * n + 1 if n == 63 else n
    h, w, b, y = bc_inputs(A, n)
    got = run_bc(h, w, b, y, n_total, ld_h, ld_dh)
    check_bc(got, bc_torch(h, w, b, y, n_total, torch.float64), bc_torch(h, w, b, y, n_total, torch.float32), n,
             "A%d-n%d-ld%d/%d-N%d" % (A, n, ld_h, ld_dh, n_total))


@pytest.mark.parametrize("A", (6, 18))
def test_bc_loss_large_logits_stay_finite(A):
    """Head weights scaled until the logits reach about +-80: exp(z) overflows fp32 without the max subtraction (NaN), and
    log(softmax) of the losing classes underflows without the log-sum-exp form."""
    n = 257
    h, w, b, y = bc_inputs(A, n, scale=13.0)
    r64, r32 = bc_torch(h, w, b, y, n, torch.float64), bc_torch(h, w, b, y, n, torch.float32)
    assert float(r64["z"].abs().max()) > 75.0
    check_bc(run_bc(h, w, b, y, n), r64, r32, n, "A%d-large" % A, key="bc_large")


def test_bc_loss_label_out_of_range_is_inert_and_arguments_are_checked():
    _l, lib = _lib()
    A, n = 6, 9
    h, w, b, y = bc_inputs(A, n)
    y[2], y[5] = float(A), -1.0
    keep = torch.ones(n, dtype=torch.bool)
    keep[2] = keep[5] = False
    got = run_bc(h, w, b, y, n)
    r64 = bc_torch(h[keep], w, b, y[keep], n, torch.float64)
    assert bool((got["dh"][~keep] == 0).all())
    assert got["correct"] == r64["correct"]
    for name, want in (("loss", r64["loss"]), ("dh", r64["dh"]), ("dw", r64["dw"]), ("db", r64["db"])):
        k = got[name][keep] if name == "dh" else got[name]
        assert float((k - want).abs().max()) <= OP_TOL * float(want.abs().max()) + 1e-7, name
    f = dict(dtype=torch.float32, device="cuda")
    x, wf = torch.zeros(4096, **f), c_int64()
    args = lambda A=6, ld=512, hp=x, n_total=4: (_p(x), _p(x), A, _p(hp), ld, 4, _p(x), n_total, _p(x), 512, _p(x), _p(x), _p(x), _p(x), _st())
    assert lib.ddrl_op_heads_bc_loss(*args(A=1)) == UNSUPPORTED and lib.ddrl_op_heads_bc_loss(*args(A=19)) == UNSUPPORTED
    assert lib.ddrl_op_heads_bc_loss(*args(ld=510)) == INVALID and lib.ddrl_op_heads_bc_loss(*args(hp=x[1:])) == INVALID
    assert lib.ddrl_op_heads_bc_loss(*args(n_total=3)) == INVALID
    assert lib.ddrl_op_heads_bc_ws_floats(19, 4, byref(wf)) == UNSUPPORTED


# ---- 2. the gather kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 5, 130))
@pytest.mark.parametrize("C", (1, 4))
def test_gather_rows_is_bit_exact(C, n):
    from ddrl4nav_amd import ops
    N = 130
    g = torch.Generator().manual_seed(C * 1000 + n)
    src = torch.randint(0, 256, (N, C, 84, 84), dtype=torch.uint8, generator=g).cuda()
    lab = (torch.arange(N, dtype=torch.float32) * 0.5 - 3.0).cuda()
    if n == 130:
        idx = torch.randperm(N, generator=g)                       # a full permutation
    elif n == 5:
        idx = torch.tensor([7, 129, 7, 0, 7])                     # repeated indices, both ends
    else:
        idx = torch.tensor([64])
    idx = idx.to(torch.int32).cuda()
    dst = torch.full((n + 1, C, 84, 84), 0xA5, dtype=torch.uint8, device="cuda")
    ldst = torch.full((n + 1,), SENT, dtype=torch.float32, device="cuda")
    ops.gather_rows_u8(src, idx, dst, lab, ldst, n)
    torch.cuda.synchronize()
    assert torch.equal(dst[:n], torch.index_select(src, 0, idx.long()))
    assert torch.equal(ldst[:n], torch.index_select(lab, 0, idx.long()))
    assert bool((dst[n:] == 0xA5).all()) and float(ldst[n]) == SENT


def test_gather_rows_bad_index_and_arguments():
    from ddrl4nav_amd import ops
    _l, lib = _lib()
    src = torch.randint(1, 256, (4, 1, 84, 84), dtype=torch.uint8).cuda()
    lab = torch.arange(4, dtype=torch.float32).cuda()
    idx = torch.tensor([2, 4, -1, 0], dtype=torch.int32).cuda()
    dst = torch.full((4, 1, 84, 84), 0xA5, dtype=torch.uint8, device="cuda")
    ldst = torch.full((4,), SENT, dtype=torch.float32, device="cuda")
    ops.gather_rows_u8(src, idx, dst, lab, ldst)
    torch.cuda.synchronize()
    assert torch.equal(dst[0], src[2]) and torch.equal(dst[3], src[0]) and bool((dst[1:3] == 0).all())
    assert ldst.cpu().tolist() == [2.0, -1.0, -1.0, 0.0]
    call = lambda s=src, d=dst, rb=7056, ls=lab, ld=ldst: lib.ddrl_op_gather_rows_u8(_p(s), 4, rb, _p(idx), 4, _p(d), _p(ls), _p(ld), _st())
    assert call(rb=7048) == INVALID and call(s=src.view(-1)[1:]) == INVALID and call(d=src) == INVALID and call(ld=None) == INVALID
    assert call(ls=None, ld=None) == 0
    torch.cuda.synchronize()


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", (6, 18))
def test_bc_loss_is_deterministic(A):
    h, w, b, y = bc_inputs(A, 257)
    a, c = run_bc(h, w, b, y, 257), run_bc(h, w, b, y, 257)
    for k in ("loss", "dh", "dw", "db"):
        assert torch.equal(a[k], c[k]), k
    assert a["correct"] == c["correct"]


# ---- the driver --------------------------------------------------------------------------------------------------------------------
C_FRAMES, A_PONG = 4, 6


def _configs(shared, n_actions=A_PONG):
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": C_FRAMES,
           "discrete_action": True, "discrete_actions": list(range(n_actions)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfgs = {"config": BaseConfig(types.SimpleNamespace(task="imit", ip="127.0.0.1"), env), "config_nn": ConfigNN(env), "config_env": env}
    cfgs["config_nn"].SHARE_CNN_NET = bool(shared)
    return cfgs


@pytest.fixture(scope="module", params=[False, True], ids=["split", "shared"])
def net(request):
    from ddrl4nav_amd.runner import create_net
    torch.manual_seed(11)
    return create_net(_configs(request.param), max_batch=64)


def write_demos(d, n_samples, seed, labels=None):
    """A demonstration directory in the reader's format (data/mimic_exp.py): one frame per file, a sample = C consecutive files.
    The Atari reader appends a line once per frame file it is the first to load, so the first line counts C times."""
    from ddrl4nav_amd.data.mimic_exp import MimicExpFactory
    d.mkdir()
    lines = n_samples - (C_FRAMES - 1)
    rng = np.random.RandomState(seed)
    for i in range(lines + C_FRAMES - 1):
        np.save(str(d / ("0_0_%d.npy" % i)), rng.randint(0, 256, (84, 84)).astype(np.uint8))
    lab = rng.randint(0, A_PONG, lines) if labels is None else labels
    with open(str(d / "dataset.txt"), "w") as f:
        f.write(str(d) + "\n")
        for i in range(lines):
            f.write(",".join("0_0_%d.npy" % (i + c) for c in range(C_FRAMES)) + "||" + str(int(lab[i])) + "\n")
    ds = MimicExpFactory().mimic_reader("atari", str(d) + "/")
    assert len(ds) == n_samples
    return ds


def kwargs(batch, epochs=1, lr=1e-4, freq=1, kind="classification"):
    return dict(imitation_learning_rate=lr, imitation_training_batch=batch, imitation_training_epoch=epochs,
                imitation_saving_frequency=freq, imitation_model_key="imitMODEL_IMITATION", imitation_training_type=kind)


class TorchActor(torch.nn.Module):
    """actor_linear(pre(x)) from torch modules (AtariPreNet's shape contract: three leaky-ReLU convolutions and a linear layer)."""

    def __init__(self, net, dtype):
        super().__init__()
        enc = "prenet." if net.prenet is not None else "actor.pre."
        sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        self.conv1, self.conv2 = torch.nn.Conv2d(C_FRAMES, 32, 8, 4), torch.nn.Conv2d(32, 64, 4, 2)
        self.conv3, self.linear, self.head = torch.nn.Conv2d(64, 64, 3, 1), torch.nn.Linear(3136, FEAT), torch.nn.Linear(FEAT, A_PONG)
        self.names = {}
        for mod, key in (("conv1", enc + "conv1"), ("conv2", enc + "conv2"), ("conv3", enc + "conv3"), ("linear", enc + "linear"),
                         ("head", "actor.actor_linear")):
            for t in ("weight", "bias"):
                getattr(self, mod)._parameters[t] = torch.nn.Parameter(sd[key + "." + t].to(dtype))
                self.names[key + "." + t] = getattr(getattr(self, mod), t)
        self.dtype = dtype

    def forward(self, x_u8):
        x = torch.from_numpy((np.asarray(x_u8, np.float64) / 255.0).astype(np.float32)).to(self.dtype)   # float32(u8 / 255.0)
        x = F.leaky_relu(self.conv3(F.leaky_relu(self.conv2(F.leaky_relu(self.conv1(x))))))
        return self.head(self.linear(x.flatten(1)))


def torch_steps(net, dtype, xs, ys, chunks, lr):
    m = TorchActor(net, dtype)
    opt = torch.optim.Adam(m.parameters(), lr)
    losses = []
    for c in chunks:
        loss = F.cross_entropy(m(xs[c]), torch.from_numpy(ys[c]).long())
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return m, losses


def dataset_arrays(ds):
    xs, ys = zip(*[ds[i] for i in range(len(ds))])
    return np.stack(xs), np.stack(ys)[:, 0]


def epoch_chunks(ds, batch, seed, epochs=1):
    from ddrl4nav_amd.data.mimic_exp import batches
    torch.manual_seed(seed)
    return [list(batches(ds, batch).iter_indices()) for _ in range(epochs)]


@pytest.mark.parametrize("n", (5, 33))
def test_one_step_matches_float64_and_leaves_the_critic_side_alone(net, tmp_path, n):
    from ddrl4nav_amd._lib import check
    hp = net.hot_path
    ds = write_demos(tmp_path / "demos", n, seed=n)
    xs, ys = dataset_arrays(ds)
    lr = 1e-3
    chunks = epoch_chunks(ds, n, seed=5)[0]
    m64, l64 = torch_steps(net, torch.float64, xs, ys, chunks, lr)
    with torch.no_grad():
        p_old = torch.softmax(TorchActor(net, torch.float64)(xs), 1).numpy()
        p_new = torch.softmax(m64(xs), 1).numpy()
    # a PPO optimiser state that is not all zeros, to be found untouched
    hp.adam_m.normal_()
    hp.adam_v.uniform_()
    check(hp.lib.ddrl_set_step(hp.ctx, 7))
    prefix = sum(p.numel() for k, p in net.named_parameters() if k in m64.names)
    before = (hp.params[prefix:].clone(), hp.adam_m.clone(), hp.adam_v.clone())
    start = hp.params.clone()
    torch.manual_seed(5)
    try:
        net.imitation_learning(ds, None, "imitUPDATE_TAG", **kwargs(n, lr=lr))
        assert len(net.imitation_log) == 1 and net.imitation_log[0][:2] == (1, 0)
        loss = net.imitation_log[0][2]
        print("one step n=%d: loss %.9g float64 %.9g" % (n, loss, l64[0]))
        assert abs(loss - l64[0]) <= 1e-5 * abs(l64[0]) + 2e-6
        acc = float((p_old.argmax(1) == ys.astype(np.int64)).mean())     # one batch = the whole set, before the step
        assert abs(net.imitation_log[0][3] - acc) < 1e-6
        assert torch.equal(hp.params[prefix:], before[0]), "critic-side parameters changed"
        assert torch.equal(hp.adam_m, before[1]) and torch.equal(hp.adam_v, before[2]) and hp.step == 7, "PPO optimiser state changed"
        assert not torch.equal(hp.params[:prefix], start[:prefix])
        # net(states) runs on the new weights: the packed layouts were rebuilt.  The step moves the probabilities by far more than
        # fp32 evaluation errs, so "new" and "old" weights are told apart with a margin of 20
        (probs, _), _ = net([torch.from_numpy(xs)], play_mode=True)
        moved = float(np.abs(p_new - p_old).max())
        assert float(np.abs(probs.cpu().numpy() - p_new).max()) <= 0.05 * moved, (moved,)
    finally:
        hp.params.copy_(start)
        hp.reset_optimizer()
        hp.params_changed()


def record_ratio(key, value):
    slot = P.MARGINS.measured.setdefault("imitation", {})
    slot[key] = max(slot.get(key, 0.0), float(value))
    try:
        P.MARGINS._flush()
    except OSError:
        pass


def test_three_steps_stay_beside_torch_fp32(net, tmp_path):
    """Per parameter tensor: |kernels - float64| / |torch fp32 - float64| (L2) after three Adam steps on the same batches, limit
    2.0 (module docstring).  The ratios are printed and logged under "imitation" in the measured-margins file."""
    hp = net.hot_path
    ds = write_demos(tmp_path / "demos", 24, seed=3)
    xs, ys = dataset_arrays(ds)
    lr = 1e-4
    chunks = epoch_chunks(ds, 8, seed=9)[0]
    assert [len(c) for c in chunks] == [8, 8, 8]
    m64, l64 = torch_steps(net, torch.float64, xs, ys, chunks, lr)
    m32, _ = torch_steps(net, torch.float32, xs, ys, chunks, lr)
    start = hp.params.clone()
    torch.manual_seed(9)
    try:
        net.imitation_learning(ds, None, "imitUPDATE_TAG", **kwargs(8, lr=lr))
        got = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    finally:
        hp.params.copy_(start)
        hp.params_changed()
    for i, row in enumerate(net.imitation_log):
        assert abs(row[2] - l64[i]) <= 1e-3 * abs(l64[i]), (i, row, l64[i])     # the same batches in the same order
    mode = "shared" if net.prenet is not None else "split"
    worst = []
    for name, p64 in m64.names.items():
        num = float((got[name] - p64.detach()).norm())
        den = float((m32.names[name].detach().double() - p64.detach()).norm())
        ratio = num / max(den, 1e-300)
        short = name.split(".")[-2] + "." + name.split(".")[-1]
        print("three steps %-6s %-22s kernel %.3e torch32 %.3e ratio %.3f" % (mode, short, num, den, ratio))
        record_ratio("param_l2_3steps_%s_%s" % (mode, short), ratio)
        worst.append((ratio, name))
    assert max(worst)[0] <= STEP_LIMIT, max(worst)


class FakePipe:
    def __init__(self, net):
        self.net, self.calls, self.blobs_match = net, [], []

    def set(self, key, blob):
        self.calls.append(("set", key))
        ok, index = True, 0
        for _, p in self.net.named_parameters():
            t, used = self.net._decode_wb(blob[index:])
            index += used
            ok = ok and torch.equal(t.to(p.device), p.data)
        self.blobs_match.append(ok and index == len(blob))

    def incr(self, key):
        self.calls.append(("incr", key))

    def execute(self):
        self.calls.append(("execute",))


def test_epoch_protocol_batches_publishing_and_log(net, tmp_path, monkeypatch):
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.data.mimic_exp import batches
    hp = net.hot_path
    ds = write_demos(tmp_path / "demos", 70, seed=4)
    xs, ys = dataset_arrays(ds)
    seen, real = [], ops.gather_rows_u8

    def spy(src, idx, dst, labels_src=None, labels_dst=None, n=None):
        seen.append(idx[:n].cpu().tolist())
        return real(src, idx, dst, labels_src, labels_dst, n)

    monkeypatch.setattr(ops, "gather_rows_u8", spy)
    pipe = FakePipe(net)
    start = hp.params.clone()
    torch.manual_seed(21)
    try:
        net.imitation_learning(ds, pipe, "imitUPDATE_TAG", **kwargs(32, epochs=3, freq=2))
    finally:
        hp.params.copy_(start)
        hp.params_changed()
    assert [len(s) for s in seen] == [32, 32, 6] * 3
    torch.manual_seed(21)
    loader, k = batches(ds, 32), 0
    for _ in range(3):
        for X, Y in loader:
            assert np.array_equal(X.numpy(), xs[seen[k]]) and np.array_equal(Y.numpy()[:, 0], ys[seen[k]])
            k += 1
    assert k == 9
    # three epochs at saving frequency 2: one publication, after epoch 2
    assert pipe.calls == [("set", "imitMODEL_IMITATION"), ("incr", "imitUPDATE_TAG"), ("execute",)] and pipe.blobs_match == [True]
    log = net.imitation_log
    assert [(e, b) for e, b, _, _ in log] == [(e, b) for e in (1, 2, 3) for b in (0, 1, 2)]
    assert all(np.isfinite(l) and l > 0 and 0.0 <= a <= 1.0 for _, _, l, a in log)


def test_refusals(net, tmp_path):
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.runner import create_net
    ds = write_demos(tmp_path / "ok", 8, seed=1)
    with pytest.raises(NotImplementedError, match="regression"):
        net.imitation_learning(ds, None, "t", **kwargs(8, kind="regression"))
    for discrete in (True, False):
        env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "input_dim": 4, "discrete_action": discrete,
               "discrete_actions": [0, 1], "act_dim": 2}
        cfg = BaseConfig(types.SimpleNamespace(task="t", ip="127.0.0.1"), env)
        cfg.TASK_TYPE = "classical"
        g = create_net({"config": cfg, "config_nn": ConfigNN(env), "config_env": env}, max_batch=8)
        with pytest.raises(NotImplementedError, match="atari only" if discrete else "Gaussian"):
            g.imitation_learning(ds, None, "t", **kwargs(8))
    bad = write_demos(tmp_path / "bad", 8, seed=2, labels=[0, 1, A_PONG, 2, 3])
    before = net.hot_path.params.clone()
    with pytest.raises(ValueError, match="label"):
        net.imitation_learning(bad, None, "t", **kwargs(8))
    assert torch.equal(net.hot_path.params, before)
