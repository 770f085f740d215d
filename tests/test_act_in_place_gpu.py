"""Acting in place on the GPU: ddrl_op_frame_slot (csrc/ftable.hip) against ddrl_op_frame_age + ddrl_op_frame_table_planes and the numpy
model, ddrl_forward_indexed -- the indirect instantiations of the fused acting kernel (csrc/act.hip) and, above 512 samples, of
conv_fwd1_planes_kernel without a sign mask -- against ddrl_forward on the materialised stacks, the kernels' clamp, and PlaneRollout with
act_in_place on against off.  The arithmetic depends on the bytes, not on their addresses: every comparison is exact (torch.equal /
np.array_equal).  Run with `-m gpu`."""
import numpy as np
import pytest
import torch

import frame_table_ref as F
import plane_pool_ref as R
from test_act_in_place_cpu import slot_model

pytestmark = pytest.mark.gpu

A = 6
SENT_F, SENT_I, SENT_B = -7.5e8, -0x5A5A5A5B, 0xA5
A1, A2, A3 = (32 * 400,), (64 * 81,), (64 * 49,)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_hot_path(max_batch, C, shared, seed=5):
    from ddrl4nav_amd.engine import HotPath
    hp = HotPath(max_batch, n_actions=A, in_channels=C, share_cnn_net=shared)
    g = torch.Generator(device="cpu").manual_seed(seed)
    hp.params.copy_(torch.randn(hp.n_params, generator=g) * 0.02)
    hp.params_changed()
    return hp


# ---- 1. the slot operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 65, 257])         # 64 envs per workgroup: part of one, one env past one, one past four
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_frame_slot_equals_age_plus_table_and_the_model(C, n):
    """Six chained steps with random reset flags (the first with prev_age NULL, one with reset NULL): age row and table equal
    ddrl_op_frame_age + ddrl_op_frame_table_planes(first = t n, n) bit for bit, and the numpy model; nothing past them is written."""
    from ddrl4nav_amd import ops
    steps, H = 6, C - 1
    rows = H + steps
    rng = np.random.default_rng(100 * C + n)
    pool = torch.empty((rows, n, 84, 84), dtype=torch.uint8, device="cuda")        # the table builder reads its shape alone
    age_s = torch.full((steps + 1, n), SENT_B, dtype=torch.uint8, device="cuda")   # the slot operator's rows (+ one that stays untouched)
    age_r = torch.full((steps + 1, n), SENT_B, dtype=torch.uint8, device="cuda")   # ddrl_op_frame_age's
    model = np.zeros((steps, n), np.uint8)
    for t in range(steps):
        reset = ((rng.random(n) < 0.35) * rng.integers(1, 256, size=n)).astype(np.uint8)
        if t == 0:
            reset[:] = 1
        if t == 3:
            reset = None                                                           # the NULL form: no env is reset
        tab = torch.full((n + 2, 4), SENT_I, dtype=torch.int32, device="cuda")
        ref = torch.full((n + 2, 4), SENT_I, dtype=torch.int32, device="cuda")
        ops.frame_slot(rows, C, t, age_s[t - 1] if t else None, dev(reset), age_s[t], tab)
        ops.frame_age(age_r[t - 1] if t else None, dev(reset), age_r[t], C)
        ops.frame_table_planes(pool, age_r[:steps], C, ref, first=t * n, n=n)
        torch.cuda.synchronize()
        model[t], want = slot_model(model[t - 1] if t else None, reset, C, H, t, n)
        assert torch.equal(age_s, age_r) and bool((age_s[t + 1:] == SENT_B).all()), t
        assert np.array_equal(age_s[t].cpu().numpy(), model[t]), t
        assert torch.equal(tab, ref) and bool((tab[n:] == SENT_I).all()), t
        assert np.array_equal(tab[:n].cpu().numpy(), want), t
        assert int(tab[:n].min()) >= 0 and int(tab[:n].max()) < rows * n
    assert model.max() == C - 1 and (C == 1 or (model[1:] == 0).any())              # saturated ages and resets both occurred


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_frame_slot_clamps_a_hostile_previous_age(C):
    """prev_age 255 at t = 0 of a pool with hist = C - 1 and no spare row: the age saturates, the look-back is clamped, no entry < 0."""
    from ddrl4nav_amd import ops
    n, rows = 65, C
    prev = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    zero = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    age, ref_age = torch.empty_like(prev), torch.empty_like(prev)
    tab, ref = torch.empty((n, 4), dtype=torch.int32, device="cuda"), torch.empty((n, 4), dtype=torch.int32, device="cuda")
    ops.frame_slot(rows, C, 0, prev, zero, age, tab)
    ops.frame_age(prev, zero, ref_age, C)
    ops.frame_table_planes(torch.empty((rows, n, 84, 84), dtype=torch.uint8, device="cuda"), ref_age, C, ref, first=0, n=n)
    want_age, want = slot_model(np.full(n, 255, np.uint8), np.zeros(n, np.uint8), C, C - 1, 0, n)
    assert torch.equal(age, ref_age) and torch.equal(tab, ref)
    assert np.array_equal(age.cpu().numpy(), want_age) and np.array_equal(tab.cpu().numpy(), want)
    assert int(tab.min()) >= 0 and np.array_equal(tab[:, 0].cpu().numpy(), np.arange(n)) and bool((age == C - 1).all())


# ---- 2. ddrl_forward_indexed against ddrl_forward on the materialised stacks ---------------------------------------------------------------
T, N = 6, 5


def plane_pool(C, t_rows=T, n_envs=N, seed=0):
    """(planes [C-1+t_rows, n_envs, 84, 84], age [t_rows, n_envs]) with resets at step 0, mid-rollout and on consecutive steps."""
    rng = np.random.default_rng(70 + C + seed)
    planes = rng.integers(0, 256, size=(C - 1 + t_rows, n_envs, 84, 84), dtype=np.uint8)
    age = np.zeros((t_rows, n_envs), np.uint8)
    for t in range(1, t_rows):
        age[t] = R.next_age(age[t - 1], (rng.random(n_envs) < 0.25).astype(np.uint8), C)
    return planes, age


def acting(hp, n, call, keep, act=None):
    """Sentinels into everything compared, then `call(outputs)`: [probs, value, action, logp, both encoders' features, a3 (and, kept,
    a1 / a2) of every encoder] as bit patterns."""
    ne = 1 if hp.cfg.share_cnn_net else 2
    if keep:   # a fused forward without the switch leaves a1 / a2 on chip and the context refuses views of them: store them once first
        call(dict(act=act) if act is not None else {})
    out = dict(probs=torch.full((n, A), SENT_F, device="cuda"), value=torch.full((n,), SENT_F, device="cuda"),
               logp=torch.full((n,), SENT_F, device="cuda"))
    if act is None:
        out["action"] = torch.full((n,), SENT_F, device="cuda")
    else:
        out["act"] = act
    views = [(2, A3)] + ([(0, A1), (1, A2)] if keep else [])
    for e in range(ne):
        for which, shape in views:
            hp.debug_view(which, shape, n, e).fill_(SENT_F)
    call(out)
    ha, hc = hp.last_features(n)
    torch.cuda.synchronize()
    got = [out["probs"], out["value"], out["logp"], ha, hc] + ([out["action"]] if act is None else [])
    for e in range(ne):
        for which, shape in views:
            got.append(hp.debug_view(which, shape, n, e).clone())
    sent = torch.tensor(SENT_F).view(torch.int32).item()
    got = [g.clone().view(torch.int32) for g in got]
    for i, g in enumerate(got):
        assert not bool((g == sent).any()), i                  # every element was written
    return got


def assert_same_forward(hp, planes_dev, tab, stacks, what, keep, act=None, seed=3):
    n = tab.shape[0]
    assert stacks.shape[0] == n and stacks.is_contiguous()
    ref = acting(hp, n, lambda o: hp.forward(stacks, seed=seed, stream_id=2, **o), keep, act)
    got = acting(hp, n, lambda o: hp.forward_indexed(planes_dev, tab, n, seed=seed, stream_id=2, **o), keep, act)
    assert len(ref) == len(got)
    for i, (x, y) in enumerate(zip(ref, got)):
        assert torch.equal(x, y), (what, keep, i)
    return ref


@pytest.mark.parametrize("shared", [0, 1], ids=["separate", "shared"])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_indexed_forward_is_bit_identical_on_the_fused_kernel(n, C, shared):
    """Tables of the plane pool (a range that crosses a step boundary; shuffled indices) and of stacked frames, with a1 / a2 on chip
    and stored, sampling and with the actions given."""
    from ddrl4nav_amd import ops
    planes, age = plane_pool(C)
    planes_dev, age_dev = dev(planes), dev(age)
    rng = np.random.default_rng(10 * n + C)
    stacked = dev(rng.integers(0, 256, size=(7, C, 84, 84), dtype=np.uint8))
    cases = []
    for what, kw in (("crossing", dict(first=1 * N + 2)), ("shuffled", dict(idx=dev(rng.integers(0, T * N, size=n).astype(np.int32))))):
        tab = ops.frame_table_planes(planes_dev, age_dev, C, torch.empty((n, 4), dtype=torch.int32, device="cuda"), n=n, **kw)
        stacks = ops.gather_frame_stacks(planes_dev, age_dev, C, torch.empty((n, C, 84, 84), dtype=torch.uint8, device="cuda"), n=n, **kw)
        assert np.array_equal(stacks.cpu().numpy(), F.frames_of(planes, tab.cpu().numpy(), C)), what
        cases.append((what, planes_dev, tab, stacks))
    sidx = rng.integers(0, 7, size=n).astype(np.int32)
    cases.append(("stacks", stacked, ops.frame_table_stacks(stacked, torch.empty((n, 4), dtype=torch.int32, device="cuda"), idx=dev(sidx)),
                  stacked[torch.from_numpy(sidx).long().cuda()].contiguous()))
    hp = make_hot_path(8, C, shared)
    try:
        for keep in (False, True):
            hp.keep_activations(keep)
            for what, src, tab, stacks in cases:
                assert_same_forward(hp, src, tab, stacks, what, keep)
        given = dev(rng.integers(0, A, size=n).astype(np.float32))
        assert_same_forward(hp, cases[1][1], cases[1][2], cases[1][3], "shuffled, actions given", True, act=given)
    finally:
        hp.close()


# ---- 3. above ACT_FUSED_MAX: conv_fwd1_planes_kernel<NE, indirect> without a sign mask ---------------------------------------------------
@pytest.mark.parametrize("C,shared", [(4, 0), (3, 1)], ids=["C4-separate", "C3-shared"])
def test_indexed_forward_is_bit_identical_above_the_fused_limit(C, shared):
    """n = 513 = 19 envs x 27 steps, one past the fused kernel's 512: an odd count whose last conv1 tile is partial; shuffled."""
    from ddrl4nav_amd import ops
    n_envs, steps = 19, 27
    n = n_envs * steps
    assert n == 513 and (n * 400) % 256 != 0
    planes, age = plane_pool(C, steps, n_envs, seed=513)
    planes_dev, age_dev = dev(planes), dev(age)
    idx = dev(np.random.default_rng(C).permutation(n).astype(np.int32))
    tab = ops.frame_table_planes(planes_dev, age_dev, C, torch.empty((n, 4), dtype=torch.int32, device="cuda"), idx=idx)
    stacks = ops.gather_frame_stacks(planes_dev, age_dev, C, torch.empty((n, C, 84, 84), dtype=torch.uint8, device="cuda"), idx=idx)
    assert np.array_equal(stacks.cpu().numpy(), F.frames_of(planes, tab.cpu().numpy(), C))
    hp = make_hot_path(n, C, shared)
    try:
        assert_same_forward(hp, planes_dev, tab, stacks, "unfused", True)          # a1 / a2 are always stored on this path
    finally:
        hp.close()


# ---- 4. the clamp ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 2])
@pytest.mark.parametrize("C", [4, 2])
def test_fused_kernel_clamps_the_table(C, n):
    """Entries -1, -2, n_planes and n_planes + 1 give what the table clamped on the host gives.  The planes are a view into the middle
    of a larger allocation with two guard planes of another byte pattern on each side: a missing clamp would read guard bytes and fail
    the comparison, not leave the allocation."""
    from ddrl4nav_amd import ops
    planes, age = plane_pool(C)
    n_planes = planes.shape[0] * N
    big = torch.full((n_planes + 4, 84, 84), 0x5A, dtype=torch.uint8, device="cuda")
    big[2:-2] = dev(planes).reshape(-1, 84, 84)
    planes_dev = big[2:-2]
    assert planes_dev.is_contiguous() and planes_dev.data_ptr() % 16 == 0
    tab = ops.frame_table_planes(planes_dev.view(planes.shape), dev(age), C, torch.empty((n, 4), dtype=torch.int32, device="cuda"),
                                 first=3, n=n)
    bad = tab.clone()
    bad[0, 0], bad[0, C - 1 if C > 1 else 1] = -1, -2
    bad[n - 1, C - 1], bad[n - 1, 0] = n_planes, n_planes + 1
    if C < 4:
        bad[n - 1, 3], bad[0, 3] = -2, n_planes + 1           # the padding entries are loaded too
    clamped = dev(F.clamp_table(bad.cpu().numpy(), n_planes))
    assert not torch.equal(clamped[:, :C], tab[:, :C])
    frames = dev(F.frames_of(planes, bad.cpu().numpy(), C))
    assert not bool((frames == 0x5A).all(dim=-1).all(dim=-1).any())               # no plane the clamped table names looks like a guard
    hp = make_hot_path(8, C, 0)
    try:
        hp.keep_activations(True)
        want = assert_same_forward(hp, planes_dev, clamped, frames, "clamped on the host", True)
        got = acting(hp, n, lambda o: hp.forward_indexed(planes_dev, bad, n, seed=3, stream_id=2, **o), True)
        for i, (x, y) in enumerate(zip(want, got)):
            assert torch.equal(x, y), i
        assert bool((big[:2] == 0x5A).all()) and bool((big[-2:] == 0x5A).all())
    finally:
        hp.close()


# ---- 5. untouched paths -------------------------------------------------------------------------------------------------------------------
def test_contiguous_acting_and_the_iteration_are_untouched_by_an_indexed_forward():
    import test_in_place_gpu as G
    from ddrl4nav_amd import ops
    C, B = 4, 5
    planes, age = plane_pool(C)
    planes_dev = dev(planes)
    tab = ops.frame_table_planes(planes_dev, dev(age), C, torch.empty((B, 4), dtype=torch.int32, device="cuda"), first=2, n=B)
    cols = G.columns(B, 99)
    frames = dev(np.random.default_rng(3).integers(0, 256, size=(B, C, 84, 84), dtype=np.uint8))
    hp = make_hot_path(8, C, 0)
    try:
        hp.keep_activations(True)      # a1 stays viewable after the fused forwards: one_iteration() writes sentinels into it

        def both():      # the iteration first: a small acting forward keeps a1 on chip, and one_iteration() writes sentinels into it
            it = G.one_iteration(hp, B, cols, lambda: hp.ppo_iter(frames, *cols))
            return [t.clone() for t in hp.forward(frames, seed=7, stream_id=1)], it
        act0, it0 = both()
        mid = [t.clone() for t in hp.forward_indexed(planes_dev, tab, B, seed=7, stream_id=1)]
        act1, it1 = both()
        for x, y in zip(act0 + it0, act1 + it1):
            assert torch.equal(x, y)
        assert not torch.equal(mid[0], act0[0])               # it did run on other frames
    finally:
        hp.close()


# ---- 6. PlaneRollout, knob on against off ---------------------------------------------------------------------------------------------------
POOLS = ("_actions", "_logps", "values", "age", "planes")


def assert_same_pools(off, on, where):
    torch.cuda.synchronize()
    for k in POOLS:
        assert torch.equal(getattr(off, k), getattr(on, k)), (where, k)


@pytest.mark.parametrize("C", [4, 2])
def test_plane_rollout_acts_in_place_bit_identically(C):
    """The three chained rollouts of tests/test_plane_pool_gpu.py (N = 3, T = 5; carry_over() then carry_over(keep_step=True)), acted on
    step by step: act(0) of the second rollout comes without a put and rebuilds its table.  One net per rollout, the same weights; the
    knob reaches the second through config_nn."""
    import test_plane_pool_gpu as P
    from ddrl4nav_amd.agent import PlaneRollout
    net_off, net_on = P.make_net(C), P.make_net(C, ACT_IN_PLACE=True)
    assert net_off.act_in_place is False and net_on.act_in_place is True
    off = PlaneRollout(net_off, P.N, horizon=P.T, channels=C, seed=11)
    on = PlaneRollout(net_on, P.N, horizon=P.T, channels=C, seed=11)
    assert off.act_in_place is False and off._stack is not None and off._stack.shape == (P.N, C, 84, 84) and off._slot_tab is None
    assert on.act_in_place is True and on._stack is None and on._slot_tab.shape == (P.N, 4)
    assert PlaneRollout(net_on, P.N, horizon=P.T, channels=C, act_in_place=False)._stack is not None     # the argument overrides the net
    for ro in (off, on):
        ro.planes.fill_(0xEE)
    rng = np.random.default_rng(77)
    rewards = dev(rng.choice(np.array([-1, 0, 1], np.float32), size=(3, P.T + 1, P.N)).astype(np.float32))
    dones = dev((rng.random((3, P.T + 1, P.N)) < 0.2).astype(np.uint8))
    for r in range(3):
        for ro in (off, on):
            P.drive(ro, r, act=True, rewards=rewards, dones=dones)
            ro.finish()
        assert_same_pools(off, on, r)
        assert torch.equal(off.adv, on.adv) and torch.equal(off.ret, on.ret)
        assert on._slot_t == P.T
        off.carry_over(**P.CLOSE[r])
        on.carry_over(**P.CLOSE[r])
        assert on._slot_t == -1 and on.t0 == off.t0
    if not P.CLOSE[2]:                                         # act(0) after the last carry_over(), again without a put
        assert torch.equal(off.act(0), on.act(0)) and on._slot_t == 0
    assert_same_pools(off, on, "end")
    assert on._stack is None                                   # nothing was gathered on the way
    for t in range(P.T + 1):
        assert torch.equal(on.stacks(t), off.stacks(t)), t
    assert on._stack is not None and on._stack.shape == (P.N, C, 84, 84)


def test_ring_fed_plane_rollout_acts_in_place_bit_identically():
    """Two chained rollouts with the knob on, fed through put_new_frames_from_ring, against direct puts with the knob off."""
    import test_plane_pool_gpu as P
    from ddrl4nav_amd.agent import PlaneRollout
    from ddrl4nav_amd.data import PinnedRing
    C = 4
    frames = P.sequence_frames()
    net = P.make_net(C)
    off = PlaneRollout(net, P.N, horizon=P.T, channels=C, seed=5)
    on = PlaneRollout(net, P.N, horizon=P.T, channels=C, seed=5, act_in_place=True)
    for ro in (off, on):
        ro.planes.fill_(0xEE)
    ring = PinnedRing(P.N * R.PLANE, n_slots=16)
    for r in range(2):
        for t in range(P.T + 1):
            if t >= 1 or r == 0:
                ring.acquire(timeout_ms=1000)[:] = frames[r, t].reshape(-1)
                ring.commit()
    zeros_r, zeros_d = torch.zeros(P.N, device="cuda"), torch.zeros(P.N, dtype=torch.uint8, device="cuda")
    for r in range(2):
        for t in range(P.T + 1):
            if t >= 1 or r == 0:
                off.put_new_frames(t, dev(frames[r, t]), reset=P.reset_arg(r, t))
                on.put_new_frames_from_ring(t, ring, reset=P.reset_arg(r, t))
            for ro in (off, on):
                ro.act(t)
                ro.record(t, zeros_r, zeros_d)
        for ro in (off, on):
            ro.finish()
        assert_same_pools(off, on, r)
        off.carry_over()
        on.carry_over()
    assert ring.pending() == 0 and on._stack is None
    ring.close()


# ---- 7. the measurement tool ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leg", ["in_place", "kernels"])
def test_act_tool_runs_one_small_leg(leg):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_act_in_place.py"), "--envs", "4", "--steps", "8", "--runs", "1",
                        "--warmup", "0", "--passes", "1", "--legs", leg], capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    res = out["passes"][0]["legs"][leg]
    if leg == "kernels":
        assert set(res["ActConvs_us_per_call"]) == {"contiguous", "indirect"} and min(res["ActConvs_us_per_call"].values()) > 0
    else:
        assert res["median_ms"] > 0 and len(res["runs_ms"]) == 1
        assert res["pool_bytes"] == {"planes": (3 + 8 + 1) * 4 * R.PLANE, "age": 9 * 4, "slot_table": 4 * 16}      # no acting scratch
