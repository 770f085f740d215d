"""Host side of partial-episode bootstrapping (tests/truncation_ref.py is the rule book): GAE with the select
against the oracle scan and against an analytic case in float64, the fleet's terminal observation anchored to the navigation env's at one
robot per world, the header against the binding table, every argument check of the four new entry points (decided before HIP), and
truncations_per_rollout.  No GPU."""
import ctypes
import types

import numpy as np
import pytest

import fleet_env_ref as F
import truncation_ref as TR
from arena_abi import A, INVALID, M, caller, common_refusals, header_declares, refused
from arena_harness import bits
from oracle import ddrl_oracle as O

NEW = ("ddrl_op_nav_env_step_final", "ddrl_op_fleet_env_step_final", "ddrl_op_file_flagged_rows", "ddrl_gae_bootstrap")


# ---- 1. GAE with the select -------------------------------------------------------------------------------------------------------------------
def gae_case(T, N, seed, p_done=0.2):
    rng = np.random.RandomState(seed)
    dones = (rng.uniform(size=(T, N)) < p_done).astype(np.uint8)
    dones[T // 2, N // 2] = 1                                           # at least one, at the smallest shape too
    return rng.normal(size=(T + 1, N)).astype(np.float32), rng.normal(size=(T, N)).astype(np.float32), dones


@pytest.mark.parametrize("T,N", [(1, 1), (5, 64), (33, 65)])
def test_without_slots_the_model_is_the_oracle_scan(T, N):
    """All slots -1 (and every boot entry a NaN): adv and ret equal oracle gae()'s bit for bit."""
    v, r, d = gae_case(T, N, T + N)
    adv, ret = TR.gae_bootstrap_ref(v, r, d, np.full((T, N), -1, np.int32), np.full((2, N), np.nan, np.float32))
    oadv, oret = O.gae(v, r, d)
    assert adv.dtype == ret.dtype == np.float32 and d.any()
    assert np.array_equal(bits(adv), bits(oadv)) and np.array_equal(bits(ret), bits(oret))
    # and a slot outside [0, S) is no slot
    wild = np.where(np.arange(T * N).reshape(T, N) % 2 == 0, 2, -7).astype(np.int32)
    adv2, ret2 = TR.gae_bootstrap_ref(v, r, d, wild, np.full((2, N), np.nan, np.float32))
    assert np.array_equal(bits(adv2), bits(oadv)) and np.array_equal(bits(ret2), bits(oret))


def test_a_constant_reward_has_no_advantage_under_its_own_value():
    """Float64, constant reward r and V = r / (1 - gamma) everywhere: with the value of the terminal observation as the successor of a
    truncated step every advantage is 0 to rounding; with the terminal treatment the truncated step's advantage is -gamma r / (1 - gamma):
    the bias the feature removes."""
    T, N, S, gamma, landa, r = 12, 3, 2, 0.99, 0.95, 0.25
    v = r / (1.0 - gamma)
    values, rewards = np.full((T + 1, N), v), np.full((T, N), r)
    dones, slots = np.zeros((T, N), np.uint8), np.full((T, N), -1, np.int32)
    for n, steps in enumerate(((3, 9), (5,), ())):                      # env 0 truncates twice, env 1 once, env 2 never
        for k, t in enumerate(steps):
            dones[t, n], slots[t, n] = 1, k
    boot = np.full((S, N), np.nan)
    boot[0, :2], boot[1, 0] = v, v                                      # only the named entries hold a value
    adv, ret = TR.gae_bootstrap_ref(values, rewards, dones, slots, boot, gamma, landa, dtype=np.float64)
    assert adv.dtype == np.float64 and np.abs(adv).max() <= 64 * np.finfo(np.float64).eps * v
    assert np.abs(ret - v).max() <= 64 * np.finfo(np.float64).eps * v
    plain, _ = TR.gae_bootstrap_ref(values, rewards, dones, np.full((T, N), -1, np.int32), boot, gamma, landa, dtype=np.float64)
    want = -gamma * r / (1.0 - gamma)
    for t, n in ((3, 0), (9, 0), (5, 1)):
        assert abs(plain[t, n] - want) <= 64 * np.finfo(np.float64).eps * v, (t, n)
    assert np.abs(plain[:, 2]).max() <= 64 * np.finfo(np.float64).eps * v and plain[2, 0] < -1.0        # and it leaks backwards


def test_file_rows_ref_counts_past_the_pool():
    info = np.array([16, 0, 16 | 1, 16, 1], np.int32)
    srcs = [np.arange(5 * 3, dtype=np.float32).reshape(5, 3), np.arange(5, dtype=np.float32).reshape(5, 1) + 100]
    dsts = [np.full((2, 5, 3), np.nan, np.float32), np.full((2, 5, 1), np.nan, np.float32)]
    count = np.array([0, 0, 1, 2, 1], np.int32)
    slot = TR.file_rows_ref(info, srcs, dsts, count)
    assert slot.tolist() == [0, -1, 1, -1, -1] and count.tolist() == [1, 0, 2, 3, 1]
    assert np.array_equal(dsts[0][0, 0], srcs[0][0]) and np.array_equal(dsts[0][1, 2], srcs[0][2]) and dsts[1][1, 2, 0] == 102
    assert np.isnan(dsts[0]).sum() == 2 * 5 * 3 - 6 and np.isnan(dsts[1]).sum() == 2 * 5 - 2


# ---- 2. the fleet's terminal observation at one robot is the navigation env's -------------------------------------------------------------------
def test_one_robot_per_world_has_the_nav_terminal_observation():
    """R = 1: before every step the nav model takes the fleet's state (tests/test_fleet_env_cpu.py anchors the two rule books that way);
    both truncate in the same steps and the fleet's observe() of `played` equals the nav model's snapshot bit for bit on those rows."""
    n = 8
    fleet, nav = F.FleetEnvRef(n, 1, seed=3, max_steps=6), TR.NavEnvFinalRef(n, seed=3, max_steps=6)
    fleet.reset()
    rng = np.random.RandomState(1)
    compared = 0
    for t in range(60):
        a = np.stack([rng.uniform(0.0, 0.6, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)
        nav.state[:] = F.nav_state(fleet.state)
        fleet.step(a)
        nav.step(a)
        final, rows = TR.fleet_final_obs(fleet)
        assert np.array_equal(rows, nav.truncated) and np.array_equal(rows, (fleet.info & TR.TRUNC_BIT) != 0)
        if rows.any():
            for x, y in zip(final, nav.final):
                assert x.dtype == y.dtype == np.float32 and np.array_equal(x[rows].view(np.int32), y[rows].view(np.int32))
            # the vector of a terminal observation: the action just played and the distance after the move, not a new episode's zeros
            s = F.nav_state(fleet.played)[rows]
            assert np.array_equal(final[1][rows, 2], s[:, 3].astype(np.float32) / 32) and (s[:, 8] == 6).all()
            compared += int(rows.sum())
    print("terminal observations compared:", compared)
    assert compared >= 40


# ---- 3. header, binding, wrappers ----------------------------------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_binds():
    from ddrl4nav_amd import ops
    header_declares(NEW, [18, 19, 11, 13])
    assert all(hasattr(ops, k) for k in ("nav_env_step_final", "fleet_env_step_final", "file_flagged_rows", "gae_bootstrap"))
    assert ops.NAV_INFO_TRUNCATED == TR.TRUNC_BIT == 16


def test_env_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses: every refusal is decided before the first HIP call.  arena_abi.common_refusals
    with the terminal buffers among the outputs, then each entry's own shapes."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    refused(caller(lib, "ddrl_op_nav_env_step_final"), common_refusals("ddrl_op_nav_env_step_final") + [dict(n=0), dict(n=-2)])
    fleet = caller(lib, "ddrl_op_fleet_env_step_final")
    refused(fleet, common_refusals("ddrl_op_fleet_env_step_final") + [dict(nw=0), dict(nw=-1), dict(nr=0), dict(nr=5), dict(nw=2 ** 30, nr=2)])
    # the plain entry point still takes a null info; the terminal render does not
    assert fleet(info=None) == INVALID


def test_filing_argument_checks_come_before_hip():
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    N, S = 8, 2
    widths = (960, 5, 6912)
    info, count, slot = A, A + M, A + 2 * M
    src = [A + (3 + k) * M for k in range(4)]
    dst = [A + (8 + k) * M for k in range(4)]

    def call(info=info, mask=16, n=N, s=S, parts=3, src=src, dst=dst, w=widths + (4,), count=count, slot=slot, arrays=(True, True, True)):
        sa = (ctypes.c_void_p * 4)(*src) if arrays[0] else None
        da = (ctypes.c_void_p * 4)(*dst) if arrays[1] else None
        wa = (ctypes.c_int32 * 4)(*w) if arrays[2] else None
        return lib.ddrl_op_file_flagged_rows(info, mask, n, s, parts, sa, da, wa, count, slot, None)

    def moved(seq, k, v):
        return [v if i == k else x for i, x in enumerate(seq)]

    bad = [dict(info=None), dict(count=None), dict(slot=None), dict(arrays=(False, True, True)), dict(arrays=(True, False, True)),
           dict(arrays=(True, True, False)), dict(mask=0), dict(n=0), dict(n=-1), dict(s=0), dict(s=-2), dict(parts=0), dict(parts=5),
           dict(parts=-1), dict(info=info + 2), dict(count=count + 1), dict(slot=slot + 2)]
    for k in range(3):
        bad += [dict(src=moved(src, k, None)), dict(dst=moved(dst, k, None)), dict(w=moved(widths + (4,), k, 0)),
                dict(w=moved(widths + (4,), k, -5)), dict(src=moved(src, k, src[k] + 2)), dict(dst=moved(dst, k, dst[k] + 1))]
        # overlaps: a pool on its own source, on another pool's last row, on the counters; a source on the counters and the slots
        last = dst[(k + 1) % 3] + (S * N - 1) * widths[(k + 1) % 3] * 4
        bad += [dict(dst=moved(dst, k, src[k])), dict(dst=moved(dst, k, src[k] + (N - 1) * widths[k] * 4)), dict(dst=moved(dst, k, last)),
                dict(dst=moved(dst, k, count)), dict(dst=moved(dst, k, slot + 4 * (N - 1))), dict(dst=moved(dst, k, info)),
                dict(src=moved(src, k, count)), dict(src=moved(src, k, slot))]
    bad += [dict(count=slot), dict(count=slot + 4 * (N - 1)), dict(count=info), dict(slot=info + 4 * (N - 1)), dict(parts=4, w=widths + (0,)),
            dict(parts=4, src=moved(src, 3, None))]
    for kw in bad:
        assert call(**kw) == INVALID, kw


def test_gae_bootstrap_argument_checks_come_before_hip():
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    T, N, S = 5, 8, 2
    names = ("values", "rewards", "dones", "slot", "boot", "adv", "ret")
    base = {k: A + i * M for i, k in enumerate(names)}
    size = dict(values=(T + 1) * N * 4, rewards=T * N * 4, dones=T * N, slot=T * N * 4, boot=S * N * 4, adv=T * N * 4, ret=T * N * 4)

    def call(s=S, t=T, n=N, **kw):
        p = dict(base, **kw)
        return lib.ddrl_gae_bootstrap(p["values"], p["rewards"], p["dones"], p["slot"], p["boot"], s, t, n, 0.99, 0.95, p["adv"], p["ret"],
                                      None)

    bad = [{k: None} for k in names] + [dict(s=0), dict(s=-1), dict(t=-1), dict(n=0), dict(n=-4)]
    bad += [{k: base[k] + 2} for k in names if k != "dones"]
    for out in ("adv", "ret"):
        for k in names:
            if k != out:
                bad += [{out: base[k]}, {out: base[k] + size[k] - 4}]
    for kw in bad:
        assert call(**kw) == INVALID, kw
    assert call(t=0) == 0                                               # nothing to do, as ddrl_gae: no launch


def test_ops_wrappers_refuse_host_tensors():
    import torch
    from ddrl4nav_amd import ops
    obs = [torch.zeros((4,) + s) for s in ops.NAV_ENV_SHAPES]
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    with pytest.raises(AssertionError):
        ops.nav_env_step_final(i32(4, 64), torch.zeros((4, 2)), obs, torch.zeros(4), torch.zeros(4, dtype=torch.uint8), i32(4), obs)
    with pytest.raises(AssertionError):
        ops.fleet_env_step_final(i32(2, 96), 2, torch.zeros((4, 2)), obs, torch.zeros(4), torch.zeros(4, dtype=torch.uint8), i32(4), obs)
    with pytest.raises(AssertionError):
        ops.file_flagged_rows(i32(4), [(obs[1], torch.zeros((2, 4, 5)))], i32(4), i32(4))
    with pytest.raises(AssertionError):
        ops.gae_bootstrap(torch.zeros((3, 4)), torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.uint8), i32(2, 4), torch.zeros((1, 4)),
                          0.99, 0.95, torch.zeros((2, 4)), torch.zeros((2, 4)))


# ---- 4. the pool depth ------------------------------------------------------------------------------------------------------------------------------
def test_truncations_per_rollout():
    """ceil(T / max_steps): an episode lasts max_steps steps at the most, so an env truncates no more often in T steps."""
    from ddrl4nav_amd.env import DeviceNavEnv, FleetNavEnv
    from ddrl4nav_amd.env.device_nav_env import truncations_per_rollout
    for T, ms, want in ((7, 3, 3), (6, 3, 2), (1, 500, 1), (256, 500, 1), (500, 500, 1), (501, 500, 2), (256, 1, 256), (12, 5, 3)):
        assert truncations_per_rollout(T, ms) == want
        for cls in (DeviceNavEnv, FleetNavEnv):
            assert cls.truncations_per_rollout(types.SimpleNamespace(max_steps=ms), T) == want
    for T, ms in ((0, 3), (-1, 3), (5, 0)):
        with pytest.raises(ValueError):
            truncations_per_rollout(T, ms)
    # and the bound holds on the rule book: 8 envs that never move truncate every third step
    nav = TR.NavEnvFinalRef(8, seed=3, max_steps=3)
    nav.reset()
    seen = np.zeros(8, int)
    for t in range(7):
        nav.step(np.zeros((8, 2), np.float32))
        seen += nav.truncated
    assert seen.max() <= truncations_per_rollout(7, 3) and seen.sum() > 0


def test_make_device_env_reads_env_final_obs(monkeypatch):
    """The config knob reaches the constructor of both envs (stubbed: no device is needed to check the plumbing)."""
    from ddrl4nav_amd.env import device_nav_env, fleet_nav_env, make_device_env
    seen = []
    monkeypatch.setattr(device_nav_env, "DeviceNavEnv", lambda *a, **k: seen.append(k) or "nav")
    monkeypatch.setattr(fleet_nav_env, "FleetNavEnv", lambda *a, **k: seen.append(k) or "fleet")
    assert make_device_env({"env_name": "DeviceNav-v0", "env_num": 4, "env_final_obs": True}) == "nav"
    assert make_device_env({"env_name": "DeviceNavFleet-v0", "env_num": 4, "agent_num_per_env": 2, "env_final_obs": True}) == "fleet"
    assert make_device_env({"env_name": "DeviceNav-v0", "env_num": 4}) == "nav"
    assert [k["emit_final_obs"] for k in seen] == [True, True, False]
