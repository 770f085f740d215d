"""Single-frame ingest on the GPU: ddrl_frame_stack_push (csrc/fstack.hip) and DeviceRollout.put_new_frames* against the deque model of
tests/test_frame_stack_cpu.py (the reference's FrameStackWrapper restated; pinned against the closed form there).  uint8 throughout:
every comparison is exact.  Run with `-m gpu`."""
import json
import os
import subprocess
import sys
import threading
import types

import numpy as np
import pytest
import torch

from ddrl4nav_amd.utils.recipe import make_weights
from test_frame_stack_cpu import PLANE, DequeStack, episode

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _model_next(prev, newest, reset):
    """One step of the deque model from an arbitrary stack `prev` [n, C, 84, 84]: the deques are loaded with prev's planes (oldest
    first), then every env appends its new frame once, or C times when its reset flag is set."""
    n, C = prev.shape[:2]
    m = DequeStack(n, C)
    for i in range(n):
        for c in range(C):
            m.step(i, prev[i, c])
        (m.reset if reset is not None and reset[i] else m.step)(i, newest[i])
    return m.obs()


def _reset_flags(kind, rng, n):
    if kind == "null":
        return None
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "ones":
        return np.ones(n, np.uint8)
    r = (rng.random(n) < 0.3).astype(np.uint8)
    return r * rng.integers(1, 256, size=n, dtype=np.uint8)      # any non-zero byte means reset


def _dev(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize("reset_kind", ["null", "zeros", "random", "ones"])
@pytest.mark.parametrize("n", [1, 7, 256, 513])
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_kernel_equals_the_deque_model(channels, n, reset_kind):
    from ddrl4nav_amd.ops import frame_stack_push
    rng = np.random.default_rng(1000 * channels + n)
    prev = rng.integers(0, 256, size=(n, channels, 84, 84), dtype=np.uint8)
    newest = rng.integers(0, 256, size=(n, 84, 84), dtype=np.uint8)
    reset = _reset_flags(reset_kind, rng, n)
    out = torch.full((n, channels, 84, 84), 0xA5, dtype=torch.uint8, device=DEV)
    frame_stack_push(_dev(prev), _dev(newest), _dev(reset), out)
    assert np.array_equal(out.cpu().numpy(), _model_next(prev, newest, reset))
    if channels == 1:   # prev is not read: None is legal
        out.fill_(0x5A)
        frame_stack_push(None, _dev(newest), _dev(reset), out)
        assert np.array_equal(out.cpu().numpy()[:, 0], newest)


@pytest.mark.parametrize("channels,n", [(1, 3), (2, 7), (3, 1), (4, 7), (4, 256)])
def test_kernel_writes_nothing_but_next(channels, n):
    """`next` lies inside a larger tensor with 4,096 guard bytes of a known pattern on both sides; the inputs are compared with
    copies taken before the call."""
    from ddrl4nav_amd.ops import frame_stack_push
    rng = np.random.default_rng(77 + n)
    G = 4096
    nbytes = n * channels * PLANE
    big = torch.full((G + nbytes + G,), 0xC3, dtype=torch.uint8, device=DEV)
    out = big[G:G + nbytes].view(n, channels, 84, 84)
    assert out.data_ptr() % 16 == 0
    prev = _dev(rng.integers(0, 256, size=(n, channels, 84, 84), dtype=np.uint8))
    newest = _dev(rng.integers(0, 256, size=(n, 84, 84), dtype=np.uint8))
    reset = _dev((rng.random(n) < 0.3).astype(np.uint8))
    keep = [t.clone() for t in (prev, newest, reset)]
    frame_stack_push(prev, newest, reset, out)
    torch.cuda.synchronize()
    assert bool((big[:G] == 0xC3).all()) and bool((big[G + nbytes:] == 0xC3).all())
    for t, k in zip((prev, newest, reset), keep):
        assert torch.equal(t, k)
    assert np.array_equal(out.cpu().numpy(), _model_next(keep[0].cpu().numpy(), keep[1].cpu().numpy(), keep[2].cpu().numpy()))


@pytest.mark.parametrize("channels", [2, 4])
def test_chain_of_pushes_follows_an_episode(channels):
    """20 pushes ping-ponging between two buffers, random dones, against the deque model after every step."""
    from ddrl4nav_amd.ops import frame_stack_push
    n, steps = 7, 20
    stacks, newest, dones = episode(np.random.default_rng(5), n, channels, steps)
    buf = [torch.zeros((n, channels, 84, 84), dtype=torch.uint8, device=DEV) for _ in range(2)]
    frame_stack_push(buf[1], _dev(newest[0]), _dev(np.ones(n, np.uint8)), buf[0])
    assert np.array_equal(buf[0].cpu().numpy(), stacks[0])
    for t in range(steps):
        src, dst = buf[t & 1], buf[(t + 1) & 1]
        frame_stack_push(src, _dev(newest[t + 1]), _dev(dones[t]), dst)
        assert np.array_equal(dst.cpu().numpy(), stacks[t + 1]), "step %d" % t


def test_wrapper_refuses_overlap_and_bad_shapes():
    from ddrl4nav_amd._lib import DdrlError
    from ddrl4nav_amd.ops import frame_stack_push
    a = torch.zeros((2, 4, 84, 84), dtype=torch.uint8, device=DEV)
    f = torch.zeros((2, 84, 84), dtype=torch.uint8, device=DEV)
    with pytest.raises(DdrlError):
        frame_stack_push(a, f, None, a)                       # prev is next
    with pytest.raises(AssertionError):
        frame_stack_push(a, f.float(), None, torch.zeros_like(a))
    with pytest.raises(AssertionError):
        frame_stack_push(a, f[:1], None, torch.zeros_like(a))


# ---- DeviceRollout ---------------------------------------------------------------------------------------------------------------

def _configs(n_actions=6):
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": 4,
           "discrete_action": True, "discrete_actions": list(range(n_actions)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    parse = types.SimpleNamespace(task="test", ip="127.0.0.1")
    return {"config": BaseConfig(parse, env), "config_nn": ConfigNN(env), "config_env": env}


@pytest.fixture(scope="module")
def net():
    from ddrl4nav_amd.runner import create_net
    n = create_net(_configs(), max_batch=128)
    n.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_weights(0).items()})
    return n


N, T, C = 8, 8, 4
POOLS = ("frames", "actions", "logps", "values", "adv", "ret")
FOUR = (False, False, True, True)      # how each rollout is closed: carry_over(keep_step=...)


def _episode(seed, horizon=T, rollouts=4):
    """One episode long enough for `rollouts` chained rollouts.  Global step g = r * horizon + t of rollout r; every rollout stores
    horizon + 1 steps and its last one is step 0 of the next."""
    rng = np.random.default_rng(seed)
    steps = rollouts * horizon + 1
    stacks, newest, dones = episode(rng, N, C, steps, p_done=0.2)
    rewards = rng.choice(np.array([-1, 0, 1], np.float32), size=(steps, N)).astype(np.float32)
    return stacks, newest, dones, rewards


def _run_pool(net, stacks, newest, dones, rewards, single, ring=None, horizon=T, keep=FOUR):
    """len(keep) chained rollouts, rollout r closed with carry_over(keep_step=keep[r]); returns the pools cloned after every finish().
    single=False feeds whole stacks from the deque model through put_frames, True the new frame of every step through put_new_frames
    (or, with a ring whose producer writes them in order, put_new_frames_from_ring) with the recorded dones as reset flags."""
    from ddrl4nav_amd.agent import DeviceRollout
    ro = DeviceRollout(net, N, horizon=horizon, channels=C, seed=11)
    snaps = []
    for r, keep_step in enumerate(keep):
        for t in range(horizon + 1):
            g = r * horizon + t
            if t > 0 or r == 0:                              # slot 0 of a later rollout was carried over
                reset = True if g == 0 else None             # None: the dones recorded for step t - 1
                if single and ring is not None:
                    ro.put_new_frames_from_ring(t, ring, reset=reset)
                elif single:
                    ro.put_new_frames(t, torch.from_numpy(newest[g]).to(DEV), reset=reset)
                else:
                    ro.put_frames(t, torch.from_numpy(stacks[g]).to(DEV))
            ro.act(t)                                        # t == horizon: the bootstrap
            if t >= ro.t0:
                ro.record(t, torch.from_numpy(rewards[g]).to(DEV), torch.from_numpy(dones[g]).to(DEV))
        ro.finish()
        torch.cuda.synchronize()
        snaps.append({k: getattr(ro, k).clone() for k in POOLS})
        ro.carry_over(keep_step=keep_step)
    return ro, snaps


def test_rollout_from_single_frames_equals_rollout_from_stacks(net):
    ep = _episode(21)
    _, a = _run_pool(net, *ep, single=False)
    ro, b = _run_pool(net, *ep, single=True)
    for r in range(4):
        assert np.array_equal(a[r]["frames"].cpu().numpy(), ep[0][r * T:r * T + T + 1]), "rollout %d: pool A is not the episode" % r
        for k in POOLS:
            assert torch.equal(a[r][k], b[r][k]), "rollout %d, %s" % (r, k)
    # misuse: ro is after carry_over(keep_step=True), t0 == 1
    f = torch.zeros((N, 84, 84), dtype=torch.uint8, device=DEV)
    assert ro.t0 == 1
    with pytest.raises(ValueError):
        ro.put_new_frames(0, f, reset=True)                  # t < t0: slot 0 was carried over as a whole step
    ro.carry_over()
    assert ro.t0 == 0
    for bad in (None, False, torch.ones(N, dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            ro.put_new_frames(0, f, reset=bad)               # slot 0 has no previous stack
    ro.put_new_frames(0, f, reset=True)


def test_put_new_frames_sources_and_reset_overrides(net):
    """Pinned-host and pageable sources go through the staging copy; a reset tensor (device uint8, host bool) overrides the recorded
    dones."""
    from ddrl4nav_amd.agent import DeviceRollout
    rng = np.random.default_rng(3)
    ro = DeviceRollout(net, N, horizon=T, channels=C, seed=1)
    f0 = rng.integers(0, 256, size=(N, 84, 84), dtype=np.uint8)
    f1 = rng.integers(0, 256, size=(N, 84, 84), dtype=np.uint8)
    f2 = rng.integers(0, 256, size=(N, 84, 84), dtype=np.uint8)
    flags = (rng.random(N) < 0.5).astype(np.uint8)
    ro.put_new_frames(0, torch.from_numpy(f0).pin_memory(), reset=True)
    s0 = _model_next(np.zeros((N, C, 84, 84), np.uint8), f0, np.ones(N, np.uint8))
    assert np.array_equal(ro.frames[0].cpu().numpy(), s0)
    ro.put_new_frames(1, f1, reset=torch.from_numpy(flags).to(DEV))          # pageable numpy source
    s1 = _model_next(s0, f1, flags)
    assert np.array_equal(ro.frames[1].cpu().numpy(), s1)
    ro.record(1, torch.zeros(N), torch.ones(N, dtype=torch.uint8))           # recorded dones say "all", the override says otherwise
    ro.put_new_frames(2, torch.from_numpy(f2).to(DEV), reset=torch.from_numpy(flags.astype(bool)))
    assert np.array_equal(ro.frames[2].cpu().numpy(), _model_next(s1, f2, flags))
    ro.put_new_frames(2, torch.from_numpy(f2).to(DEV), reset=False)
    assert np.array_equal(ro.frames[2].cpu().numpy(), _model_next(s1, f2, None))
    ro.put_new_frames(2, torch.from_numpy(f2).to(DEV))                       # None: the dones recorded for step 1
    assert np.array_equal(ro.frames[2].cpu().numpy(), _model_next(s1, f2, np.ones(N, np.uint8)))


@pytest.mark.parametrize("horizon,keep", [(32, (False,)), (8, FOUR)], ids=["one_rollout_T32", "four_rollouts_T8"])
def test_ring_of_single_frames_fills_the_same_pool(net, horizon, keep):
    """A producer thread writes the 33 single-frame slots of the episode (T + 1 of one rollout with T = 32; 4 * T + 1 of four chained
    ones with T = 8, where the first ring put of the later rollouts is slot 1) into a two-slot pinned ring as fast as slots free up; the
    consumer calls put_new_frames_from_ring + act per step.  The pool equals the one fed whole stacks.  One run, no repetition; every
    wait has a timeout."""
    from ddrl4nav_amd.data import PinnedRing
    ep = _episode(22 + horizon, horizon, len(keep))
    newest = ep[1]
    slots = len(keep) * horizon + 1
    assert slots == 33
    _, a = _run_pool(net, *ep, single=False, horizon=horizon, keep=keep)
    ring = PinnedRing(N * PLANE, n_slots=2)
    err = []

    def producer():
        try:
            for g in range(slots):
                buf = ring.acquire(timeout_ms=20000)
                buf[:] = newest[g].reshape(-1)
                ring.commit()
        except Exception as e:
            err.append(e)

    th = threading.Thread(target=producer, daemon=True)
    th.start()
    try:
        _, b = _run_pool(net, *ep, single=True, ring=ring, horizon=horizon, keep=keep)
    finally:
        th.join(timeout=30)
    assert not th.is_alive() and not err, err
    assert ring.pending() == 0
    ring.close()
    for r in range(len(keep)):
        for k in POOLS:
            assert torch.equal(a[r][k], b[r][k]), "rollout %d, %s" % (r, k)


def test_ingest_tool_runs_small():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_ingest_frames.py"), "--envs", "8", "--steps", "4",
                        "--rollouts", "2"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    legs = ("full_serial", "single_serial", "full_overlap", "single_overlap")
    for leg in legs:
        assert out[leg]["median_ms"] > 0 and out[leg]["p95_ms"] >= out[leg]["median_ms"]
    for mode in ("serial", "overlap"):
        assert out["full_" + mode]["bytes_per_step"] == 4 * out["single_" + mode]["bytes_per_step"] == 4 * 8 * PLANE
