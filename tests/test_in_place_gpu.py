"""Learning in place on the GPU: the frame-table builders (csrc/ftable.hip) against the numpy model of tests/frame_table_ref.py,
ddrl_ppo_iter_indexed -- the indirect instantiations of the three conv1 kernels -- against ddrl_ppo_iter on the materialised frames,
the kernels' clamp, and PPO.learn with config_nn.FRAMES_IN_PLACE against the staged path.  The arithmetic depends on the bytes, not on
their addresses: every comparison is exact (torch.equal; sign masks and activations as int32 bit patterns).  Run with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

import frame_table_ref as F
import plane_pool_ref as R

pytestmark = pytest.mark.gpu

N, T, A = 3, 5, 6
SENT_F, SENT_I = -7.5e8, -0x5A5A5A5B
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the builders against the model -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(C, hostile=False):
    """(planes [C-1+T, N, 84, 84], age [T, N], columns [4, T N]) of the learner's rows: resets (age 0) at step 0, mid-rollout and on
    consecutive steps of env 0; hostile: 255 in every age byte."""
    rng = np.random.default_rng(60 + C)
    planes = rng.integers(0, 256, size=(C - 1 + T, N, 84, 84), dtype=np.uint8)
    age = np.zeros((T, N), np.uint8)
    for t in range(1, T):
        age[t] = R.next_age(age[t - 1], np.array([t in (2, 3), t == 3, 0], np.uint8), C)
    if hostile:
        age[:] = 255
    cols = rng.normal(size=(4, T * N)).astype(np.float32)
    return planes, age, cols


def build(C, how, idx=None, first=0, n=None, cols=None, affine=None, hostile=False):
    """One builder call into sentinel-filled destinations: (tab int32 [n, 4] on the device, columns [4][n] or None)."""
    from ddrl4nav_amd import ops
    planes, age, _ = pool(C, hostile)
    n = len(idx) if n is None else n
    tab = torch.full((n + 2, 4), SENT_I, dtype=torch.int32, device="cuda")
    dst = [torch.full((n + 2,), SENT_F, dtype=torch.float32, device="cuda") for _ in range(4)] if cols is not None else None
    src = None if cols is None else [dev(c) for c in cols]
    if how == "planes":
        ops.frame_table_planes(dev(planes), dev(age), C, tab, idx=dev(idx), first=first, n=n, columns=src, columns_dst=dst, adv_affine=affine)
    else:
        stacked = torch.empty((7, C, 84, 84), dtype=torch.uint8, device="cuda")
        ops.frame_table_stacks(stacked, tab, idx=dev(idx), first=first, n=n, columns=src, columns_dst=dst, adv_affine=affine)
    torch.cuda.synchronize()
    assert bool((tab[n:] == SENT_I).all()) and (cols is None or all(bool((c[n:] == SENT_F).all()) for c in dst))
    return tab[:n], None if cols is None else [c[:n] for c in dst]


def wild_idx(B, C):
    idx = np.random.default_rng(C).permutation(B).astype(np.int32)
    idx = np.concatenate([idx, idx[:3]])                      # duplicates
    idx[1], idx[4], idx[6], idx[9] = -1, B, I32_MAX, I32_MIN  # clamped: sample 0, B - 1, B - 1, 0
    return idx


@pytest.mark.parametrize("how", ["planes", "stacks"])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_builders_equal_the_model_and_the_gathers_columns(C, how):
    """Tables exact against the numpy model; columns and the fused affine bit-identical to ddrl_op_gather_minibatch on the clamped
    indices; a repeat gives the same bits."""
    from ddrl4nav_amd import ops
    planes, age, cols = pool(C)
    B = T * N if how == "planes" else 7
    cols = cols[:, :B]
    idx = wild_idx(B, C)
    want = F.table_planes(age, C, C - 1, N, idx) if how == "planes" else F.table_stacks(B, C, idx)
    affine = dev(np.array([0.25, 1.75], np.float32))
    rows = torch.zeros((B, 16), dtype=torch.uint8, device="cuda")        # any rows: the reference gather is asked for its columns
    for af in (None, affine):
        tab, got_c = build(C, how, idx=idx, cols=cols, affine=af)
        assert np.array_equal(tab.cpu().numpy(), want)
        ref_c = [torch.full((len(idx),), SENT_F, dtype=torch.float32, device="cuda") for _ in range(4)]
        ops.gather_minibatch(rows, dev(F.clamp_samples(idx, B).astype(np.int32)), torch.empty((len(idx), 16), dtype=torch.uint8, device="cuda"),
                             [dev(c) for c in cols], ref_c, adv_affine=af)
        for k in range(4):
            assert torch.equal(got_c[k], ref_c[k]), k
    again, _ = build(C, how, idx=idx)                                     # the table alone: the columns are optional; a repeat
    assert torch.equal(again, tab)
    # contiguous ranges, one running past either end (clamped)
    for first, n in ((0, B), (4, 3), (B - 2, 5), (-2, 4)):
        tab, got_c = build(C, how, first=first, n=n, cols=cols)
        b = first + np.arange(n)
        assert np.array_equal(tab.cpu().numpy(), F.table_planes(age, C, C - 1, N, b) if how == "planes" else F.table_stacks(B, C, b)), first
        for k in range(4):
            assert got_c[k].cpu().numpy().tobytes() == cols[k][F.clamp_samples(b, B)].tobytes()


def test_hostile_age_is_clamped_by_the_rule():
    """255 in every age byte: the full window of C - 1 steps back, never a plane below 0."""
    C = 4
    planes, age, _ = pool(C, hostile=True)
    tab, _ = build(C, "planes", first=0, n=T * N, hostile=True)
    want = F.table_planes(age, C, C - 1, N, np.arange(T * N))
    assert np.array_equal(tab.cpu().numpy(), want) and want.min() == 0
    b = np.arange(T * N)
    assert np.array_equal(want[:, 0], (b // N) * N + b % N)


# ---- 2. ddrl_ppo_iter_indexed against ddrl_ppo_iter on the materialised frames ----------------------------------------------------------
def columns(B, seed):
    rng = np.random.default_rng(seed)
    return [dev(rng.integers(0, A, size=B).astype(np.float32)), dev(-rng.random(B).astype(np.float32) - 0.5),
            dev(rng.normal(size=B).astype(np.float32)), dev(rng.normal(size=B).astype(np.float32))]


def make_hot_path(max_batch, C, shared, seed=5):
    from ddrl4nav_amd.engine import HotPath
    hp = HotPath(max_batch, n_actions=A, in_channels=C, share_cnn_net=shared)
    g = torch.Generator(device="cpu").manual_seed(seed)
    hp.params.copy_(torch.randn(hp.n_params, generator=g) * 0.02)
    hp.params_changed()
    return hp


def one_iteration(hp, B, cols, call):
    """Sentinels into everything compared, then `call`: (grad arena with its 8-float tail, a1 and m1 of every encoder as bit patterns,
    the diagnostics row)."""
    ne = 1 if hp.cfg.share_cnn_net else 2
    hp.grads.fill_(SENT_F)
    for e in range(ne):
        hp.debug_view(0, (32 * 400,), B, e).fill_(SENT_F)
        hp.debug_view(10, (400,), B, e).fill_(SENT_F)
    call()
    diag = hp.ppo_diag(cols[0], cols[1], cols[3]).clone()
    torch.cuda.synchronize()
    out = [hp.grads.clone().view(torch.int32), diag.view(torch.int64)]
    for e in range(ne):
        out.append(hp.debug_view(0, (32 * 400,), B, e).clone().view(torch.int32))
        out.append(hp.debug_view(10, (400,), B, e).clone().view(torch.int32))
    return out


def assert_same_iteration(hp, planes_dev, tab_dev, C, cols, what):
    """ppo_iter_indexed(planes, tab) against ppo_iter on the frames the table names (gathered by torch, not by a kernel under test)."""
    B = tab_dev.shape[0]
    flat = planes_dev.reshape(-1, 84, 84)
    frames = flat[tab_dev[:, :C].long().clamp(0, flat.shape[0] - 1)].contiguous()
    assert frames.shape == (B, C, 84, 84)
    ref = one_iteration(hp, B, cols, lambda: hp.ppo_iter(frames, *cols))
    got = one_iteration(hp, B, cols, lambda: hp.ppo_iter_indexed(planes_dev, tab_dev, *cols))
    names = ["grads", "diag"] + ["%s[%d]" % (k, e) for e in range((len(ref) - 2) // 2) for k in ("a1", "m1")]
    sent = torch.tensor(SENT_F).view(torch.int32).item()
    for name, x, y in zip(names, ref, got):
        if name != "diag":
            assert bool((x != sent).any()) and bool((y != sent).any()), (what, name)      # both calls wrote it
        assert torch.equal(x, y), (what, name)
    return ref, frames


# B = 1, 2, 3, 5, 7 on conv_fwd1_planes_kernel: one sample, a pair, odd tails, tiles that straddle two samples (400 pixels per sample,
# 256 per tile).  The context holds 8 samples, so conv1's weight gradient runs 4 splits of one sample pair each (WgradSplit: with
# B <= max_batch <= 1,024 a split's share is one pair or none): B = 7 fills all four with an odd tail, B = 5 leaves the last one with
# nothing, B = 1 the last three.
SMALL_B = (1, 2, 3, 5, 7)


@pytest.mark.parametrize("shared", [0, 1], ids=["separate", "shared"])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_indexed_iteration_is_bit_identical_small_batches(C, shared):
    planes, age, _ = pool(C)
    planes_dev = dev(planes)
    stacked = np.random.default_rng(80 + C).integers(0, 256, size=(7, C, 84, 84), dtype=np.uint8)
    stacked_dev = dev(stacked)
    hp = make_hot_path(8, C, shared)
    try:
        for B in SMALL_B:
            cols = columns(B, 10 * B + C)
            rng = np.random.default_rng(B)
            shuffled = rng.integers(0, T * N, size=B).astype(np.int32)
            if B >= 2:
                shuffled[-1] = shuffled[0]                    # a duplicate
            tabs = {"planes-shuffled": build(C, "planes", idx=shuffled)[0],
                    "planes-contiguous": build(C, "planes", first=4, n=B)[0],
                    "stacks-shuffled": build(C, "stacks", idx=rng.integers(0, 7, size=B).astype(np.int32))[0]}
            for what, tab in tabs.items():
                src = stacked_dev if what.startswith("stacks") else planes_dev
                assert_same_iteration(hp, src, tab.contiguous(), C, cols, (what, B))
    finally:
        hp.close()


@pytest.mark.parametrize("C,shared", [(4, 0), (3, 1)], ids=["C4-separate", "C3-shared"])
def test_indexed_iteration_is_bit_identical_on_the_resident_kernel(C, shared):
    """B = 1,311 = 19 envs x 69 steps: the smallest batch that takes conv_fwd1_resident_kernel (B * 400 >= 256 * 2048); odd, and its
    last tile is partial.  The table is the plane pool's, shuffled with duplicates.  The kernels' clamp rides along: entries overwritten
    with -1 and n_planes give what the host-clamped table gives."""
    n_envs, steps = 19, 69
    B = n_envs * steps
    assert B * 400 >= 256 * 2048 > (B - 1) * 400 and B % 2 == 1 and (B * 400) % 256 != 0
    from ddrl4nav_amd import ops
    rng = np.random.default_rng(1311 + C)
    n_planes = (C - 1 + steps) * n_envs
    big = torch.from_numpy(rng.integers(0, 256, size=(n_planes + 2, 84, 84), dtype=np.uint8)).cuda()   # a guard plane on each side
    planes_dev = big[1:-1].view(C - 1 + steps, n_envs, 84, 84)
    age = rng.integers(0, C, size=(steps, n_envs)).astype(np.uint8)
    idx = rng.integers(0, B, size=B).astype(np.int32)
    tab = torch.empty((B, 4), dtype=torch.int32, device="cuda")
    ops.frame_table_planes(planes_dev, dev(age), C, tab, idx=dev(idx))
    assert np.array_equal(tab.cpu().numpy(), F.table_planes(age, C, C - 1, n_envs, idx))
    cols = columns(B, C)
    hp = make_hot_path(B, C, shared)
    try:
        assert_same_iteration(hp, planes_dev, tab, C, cols, "valid")
        bad = tab.clone()
        hit = torch.from_numpy(rng.random((B, 4)) < 0.05).cuda()
        bad[hit] = torch.where(torch.from_numpy(rng.random(int(hit.sum())) < 0.5).cuda(), -1, n_planes).to(torch.int32)
        bad[0, 0], bad[B - 1, 3], bad[B - 1, 0] = n_planes, -1, n_planes     # the first and the odd tail's sample for certain
        clamped = dev(F.clamp_table(bad.cpu().numpy(), n_planes))
        assert not torch.equal(clamped, tab)
        want = one_iteration(hp, B, cols, lambda: hp.ppo_iter_indexed(planes_dev, clamped, *cols))
        got = one_iteration(hp, B, cols, lambda: hp.ppo_iter_indexed(planes_dev, bad, *cols))
        for x, y in zip(want, got):
            assert torch.equal(x, y)
    finally:
        hp.close()


# ---- 3. the clamp ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 2])
@pytest.mark.parametrize("C", [4, 2])
def test_kernels_clamp_the_table(C, B):
    """A valid table with entries overwritten by -1 and n_planes equals the table clamped on the host.  The planes are carved out of a
    larger allocation with a guard plane on each side: even a missing clamp would stay inside the allocation."""
    planes, age, _ = pool(C)
    n_planes = planes.shape[0] * N
    big = torch.full((n_planes + 2, 84, 84), 0x5A, dtype=torch.uint8, device="cuda")
    big[1:-1] = dev(planes).reshape(-1, 84, 84)
    planes_dev = big[1:-1]
    tab = build(C, "planes", first=3, n=B)[0].contiguous()
    bad = tab.clone()
    bad[0, 0], bad[B - 1, C - 1], bad[B - 1, 3], bad[B // 2, 0] = -1, n_planes, -1, n_planes
    clamped = dev(F.clamp_table(bad.cpu().numpy(), n_planes))
    assert not torch.equal(clamped[:, :C], tab[:, :C])
    cols = columns(B, B + C)
    hp = make_hot_path(8, C, 0)
    try:
        want, frames = assert_same_iteration(hp, planes_dev, clamped, C, cols, "clamped on the host")
        assert np.array_equal(frames.cpu().numpy(), F.frames_of(planes, bad.cpu().numpy(), C))
        got = one_iteration(hp, B, cols, lambda: hp.ppo_iter_indexed(planes_dev, bad, *cols))
        for x, y in zip(want, got):
            assert torch.equal(x, y)
        assert bool((big[0] == 0x5A).all()) and bool((big[-1] == 0x5A).all())
    finally:
        hp.close()


# ---- 4. PPO.learn with the knob on against the knob off -----------------------------------------------------------------------------------
def run_learn(net, exp):
    out = []
    for ld, update_time, last in net.learn(exp):
        assert last is True
        out.append(({k: v for k, v in ld.items() if k != "PpoBackUpTime"}, update_time))
    return out


@pytest.mark.parametrize("source", ["PlaneRollout", "DeviceRollout"])
@pytest.mark.parametrize("C", [4, 2])
@pytest.mark.parametrize("knobs", ["defaults", "K3-shuffled", "K2-in-order-minibatch-norm", "defaults-deferred"])
def test_learning_in_place_is_bit_identical(knobs, C, source):
    """The four knob settings of tests/test_plane_pool_gpu.py, the batch of each pool (B = 15): every loss dict, parameter and optimiser
    moment after learn() is the same bits with FRAMES_IN_PLACE on and off, and with it on no frame is staged."""
    import test_plane_pool_gpu as P
    a, b, _ = P.rollouts(C)
    exp = (b if source == "PlaneRollout" else a).batch()
    opts = P.KNOBS[knobs]
    off, on = P.make_net(C, seed=3, iters=2, **opts), P.make_net(C, seed=3, iters=2, FRAMES_IN_PLACE=True, **opts)
    assert off.frames_in_place is False and on.frames_in_place is True
    before = off.hot_path.params.clone()
    items_off, items_on = run_learn(off, exp), run_learn(on, exp)
    assert len(items_off) == 2 * opts.get("PPO_MINIBATCHES", 1)
    assert items_off == items_on                              # floats compared with ==: the same bits
    h0, h1 = off.hot_path, on.hot_path
    assert h0.step == h1.step == len(items_off) and off.update_time == on.update_time
    for k in ("params", "adam_m", "adam_v"):
        assert torch.equal(getattr(h0, k), getattr(h1, k)), k
    assert not torch.equal(h0.params, before)
    planes = source == "PlaneRollout"
    assert on._plane_batch is None
    if knobs.startswith("defaults"):
        assert on._mb_stage is None and off._mb_stage is None
        assert (off._plane_batch is not None) == planes                                   # as the existing test pins the default path
        assert (on._frame_tab is not None) == planes and (not planes or on._frame_tab.shape == (T * N, 4))
    else:
        assert on._mb_stage.frames is None and off._mb_stage.frames.shape[1:] == (C, 84, 84) and off._mb_stage.tab is None
        assert on._mb_stage.tab.shape == (5 if "K3" in knobs else 8, 4)                  # the largest minibatch of 15 samples


# ---- 5. untouched kernels ----------------------------------------------------------------------------------------------------------------
def test_acting_and_the_contiguous_iteration_are_untouched_by_an_indexed_one():
    C, B = 4, 5
    planes, age, _ = pool(C)
    planes_dev = dev(planes)
    tab = build(C, "planes", first=2, n=B)[0].contiguous()
    cols = columns(B, 99)
    frames = dev(np.random.default_rng(3).integers(0, 256, size=(B, C, 84, 84), dtype=np.uint8))
    hp = make_hot_path(8, C, 0)
    try:
        def both():      # the iteration first: a small acting forward keeps a1 on chip, and one_iteration() writes sentinels into it
            it = one_iteration(hp, B, cols, lambda: hp.ppo_iter(frames, *cols))
            return [t.clone() for t in hp.forward(frames, seed=7, stream_id=1)], it
        act0, it0 = both()
        hp.ppo_iter_indexed(planes_dev, tab, *cols)
        act1, it1 = both()
        for x, y in zip(act0 + it0, act1 + it1):
            assert torch.equal(x, y)
    finally:
        hp.close()
