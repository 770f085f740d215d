"""The device environments on the GPU (csrc/denv.hip, ddrl4nav_amd.env, runner/device_loop.py) against the integer model of
tests/device_env_ref.py: every state word, frame byte, reward and done after every step, bit for bit; then the closed loop -- a
PlaneRollout driven by collect() with in-pool rendering against a DeviceRollout fed by the host model -- down to every parameter after
net.learn.  Run with `-m gpu`."""
import functools
import types

import numpy as np
import pytest
import torch

import device_env_ref as R

pytestmark = pytest.mark.gpu

A = 6


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ---- 1. bit parity with the model -----------------------------------------------------------------------------------------------------------
# (game, N, n_actions, env0); the first case of each game is the coverage trajectory itself (test_device_env_cpu.py)
CASES = [("pong", 8, 6, 0), ("pong", 1, 6, 0), ("pong", 5, 2, 3), ("pong", 67, 18, 1000),
         ("catch", 6, 6, 0), ("catch", 1, 2, 0), ("catch", 67, 18, 2 ** 32 - 67)]


@functools.lru_cache(maxsize=None)
def reference(game, n, n_actions, env0):
    """(model kwargs, actions [steps][n], first frame, per-step states / frames / rewards / dones stacked) of one case; never modified."""
    seed = R.COVERAGE_SEEDS[game]
    kw, actions = R.coverage_run(game, seed)
    if (n, n_actions) != (kw["n_envs"], 6):
        actions = np.random.default_rng(seed + n).integers(0, n_actions, size=(len(actions), n)).astype(np.float32)
    kw = dict(kw, n_envs=n, n_actions=n_actions, env0=env0)
    counts, trace, first = R.play(R.DeviceEnvRef(game, **kw), actions)
    if env0 == 0 and (n, n_actions) == (R.coverage_run(game, seed)[0]["n_envs"], 6):
        assert all(counts[k] >= 1 for k in R.COVERAGE_EVENTS[game]), counts
    return kw, actions, first, tuple(np.stack([step[j] for step in trace]) for j in range(4))


def play_on_device(game, kw, actions):
    """The trajectory on a fresh DeviceEnv, every step rendered into its own row of one buffer (frame_out into a slice of a larger
    buffer) with a guard row on either side; one read-back at the end."""
    from ddrl4nav_amd.env import DeviceEnv
    steps, n = actions.shape
    env = DeviceEnv(game, device="cuda", **kw)
    env.state.fill_(-12345)                                             # reset reads nothing of what was there
    frames = torch.full((steps + 3, n, 84, 84), 0x5A, dtype=torch.uint8, device="cuda")
    states = torch.empty((steps, n, 16), dtype=torch.int32, device="cuda")
    rewards = torch.empty((steps, n), dtype=torch.float32, device="cuda")
    dones = torch.empty((steps, n), dtype=torch.uint8, device="cuda")
    acts = dev(actions)
    out = env.reset(frame_out=frames[1])
    assert out.data_ptr() == frames[1].data_ptr()
    for t in range(steps):
        f, r, d = env.step(acts[t], frame_out=frames[t + 2])
        assert f.data_ptr() == frames[t + 2].data_ptr() and r is env.reward and d is env.done
        states[t].copy_(env.state)
        rewards[t].copy_(r)
        dones[t].copy_(d)
    torch.cuda.synchronize()
    return host(frames), host(states), host(rewards), host(dones)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-N%d-A%d-env0_%d" % c)
def test_every_step_equals_the_model(case):
    game, n, n_actions, env0 = case
    kw, actions, first, (want_s, want_f, want_r, want_d) = reference(*case)
    frames, states, rewards, dones = play_on_device(game, kw, actions)
    assert (frames[0] == 0x5A).all() and (frames[-1] == 0x5A).all()      # nothing outside the rows that were handed over
    assert np.array_equal(frames[1], first)
    for t in range(len(actions)):                                       # the first step that differs, if any, names itself
        assert np.array_equal(states[t], want_s[t]), (t, states[t], want_s[t])
        assert np.array_equal(rewards[t], want_r[t]) and np.array_equal(dones[t], want_d[t]), t
        assert np.array_equal(frames[t + 2], want_f[t]), t
    assert want_d.sum() > 0 and (want_r != 0).any()


@pytest.mark.parametrize("game", ["pong", "catch"])
def test_repeats_are_bit_identical(game):
    case = CASES[0] if game == "pong" else CASES[4]
    kw, actions, _, _ = reference(*case)
    a, b = play_on_device(game, kw, actions[:100]), play_on_device(game, kw, actions[:100])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_the_env_owns_its_outputs_by_default():
    from ddrl4nav_amd.env import DeviceEnv
    kw, actions, first, (want_s, want_f, want_r, want_d) = reference(*CASES[0])
    env = DeviceEnv("pong", device="cuda", **kw)
    assert env.reset() is env.frame and np.array_equal(host(env.frame), first)
    for t in range(25):
        f, r, d = env.step(dev(actions[t]))
        assert f is env.frame and f.dtype == torch.uint8 and tuple(f.shape) == (8, 84, 84)
        assert r.dtype == torch.float32 and d.dtype == torch.uint8
    assert np.array_equal(host(f), want_f[24]) and np.array_equal(host(env.state), want_s[24])


@pytest.mark.parametrize("game", ["pong", "catch"])
def test_masked_reset(game):
    """Only the envs with a non-zero mask byte restart (all counters zero, their first frame rendered); the others keep their state
    and their rows of the frame, whatever those hold."""
    from ddrl4nav_amd.env import DeviceEnv
    n = 5
    model = R.DeviceEnvRef(game, n, seed=9, env0=2)
    env = DeviceEnv(game, n, device="cuda", seed=9, env0=2)
    model.reset()
    env.reset()
    rng = np.random.default_rng(4)
    for t in range(30):
        a = rng.integers(0, 6, n).astype(np.float32)
        model.step(a)
        env.step(dev(a))
    mask = np.array([0, 3, 0, 1, 255], np.uint8)
    before = model.state.copy()
    want = model.reset(mask)
    env.frame.fill_(0x11)
    got = env.reset(mask=dev(mask))
    assert np.array_equal(host(env.state), model.state) and np.array_equal(model.state[[0, 2]], before[[0, 2]])
    assert (model.state[[1, 3, 4], R.STEPS] == 0).all() and (model.state[[1, 3, 4], R.EVENTS] == 1).all()
    g = host(got)
    assert np.array_equal(g[[1, 3, 4]], want[[1, 3, 4]]) and (g[[0, 2]] == 0x11).all()
    a = rng.integers(0, 6, n).astype(np.float32)                        # and the game goes on for all five
    f, r, d = model.step(a)
    env.step(dev(a))
    assert np.array_equal(host(env.state), model.state) and np.array_equal(host(env.frame), f)


def test_hostile_actions_are_noops():
    """NaN, +-inf, -1, 6.0 and 1e30 leave the paddle where it is; 2.5 truncates to 2, the positive direction."""
    from ddrl4nav_amd.env import DeviceEnv
    hostile = np.array([np.nan, np.inf, -np.inf, -1.0, 6.0, 1e30, 2.5], np.float32)
    for game, speed in (("pong", 3), ("catch", 4)):
        model = R.DeviceEnvRef(game, 7, seed=2)
        env = DeviceEnv(game, 7, device="cuda", seed=2)
        model.reset()
        env.reset()
        start = model.state[:, R.PA].copy()
        for t in range(6):
            f, r, d = model.step(hostile)
            gf, gr, gd = env.step(dev(hostile))
            assert np.array_equal(host(env.state), model.state) and np.array_equal(host(gf), f)
            assert np.array_equal(host(gr), r) and np.array_equal(host(gd), d)
            assert not d.any()
        assert np.array_equal(model.state[:6, R.PA], start[:6]) and model.state[6, R.PA] == start[6] + 6 * speed


def test_state_dict_resumes_bit_identically():
    from ddrl4nav_amd.env import DeviceEnv
    kw, actions, _, (want_s, want_f, want_r, want_d) = reference(*CASES[0])
    env = DeviceEnv("pong", device="cuda", **kw)
    env.reset()
    for t in range(150):
        env.step(dev(actions[t]))
    sd = env.state_dict()
    assert not sd["state"].is_cuda and sd["game"] == "pong" and sd["points"] == 2
    other = DeviceEnv("pong", device="cuda", **kw)
    other.load_state_dict(sd)
    for t in range(150, 260):
        a = dev(actions[t])
        f0, r0, d0 = env.step(a)
        f1, r1, d1 = other.step(a)
        assert torch.equal(env.state, other.state) and torch.equal(f0, f1) and torch.equal(r0, r1) and torch.equal(d0, d1)
        assert np.array_equal(host(other.state), want_s[t]) and np.array_equal(host(f1), want_f[t])
    with pytest.raises(ValueError):
        DeviceEnv("pong", device="cuda", **dict(kw, points=3)).load_state_dict(sd)
    with pytest.raises(ValueError):
        DeviceEnv("catch", device="cuda", **kw).load_state_dict(sd)


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from ddrl4nav_amd import ops
    from ddrl4nav_amd._lib import DdrlError
    from ddrl4nav_amd.env import DeviceEnv, make_device_env
    env = make_device_env({"env_name": "DeviceCatch-v0", "env_num": 3, "discrete_actions": [0, 1, 2], "env_seed": 5, "env_max_steps": 50})
    assert (env.game, env.N, env.n_actions, env.seed, env.max_steps, env.points) == ("catch", 3, 3, 5, 50, 21)
    flat = torch.zeros(3 * R.PLANE + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(AssertionError):
        env.reset(frame_out=flat[8:8 + 3 * R.PLANE].view(3, 84, 84))    # a base that is not 16-byte aligned
    env.reset(frame_out=flat[16:16 + 3 * R.PLANE].view(3, 84, 84))
    with pytest.raises(AssertionError):
        env.step(torch.zeros(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(AssertionError):
        env.step(torch.zeros(4, dtype=torch.float32, device="cuda"))
    with pytest.raises(AssertionError):
        env.reset(frame_out=torch.zeros((2, 84, 84), dtype=torch.uint8, device="cuda"))
    with pytest.raises(AssertionError):
        env.reset(mask=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(DdrlError):                                       # the reward inside the frame
        ops.env_step("catch", env.state, torch.zeros(3, device="cuda"), env.frame, env.frame.view(-1)[:12].view(torch.float32), env.done)
    with pytest.raises(DdrlError):
        ops.env_step("catch", env.state, torch.zeros(3, device="cuda"), env.frame, env.reward, env.done, n_actions=19)


# ---- 2. the closed loop -----------------------------------------------------------------------------------------------------------------------
N, T, C = 8, 16, 4
ENV_KW = dict(seed=31, points=1, max_steps=25)                          # every env is done by step 25 at the latest: both rollouts see dones


def make_net(seed=0, share=None, iters=1):
    """The Atari PPO net with C stacked frames and A = 6 actions through create_net, recipe weights loaded."""
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.runner import create_net
    from ddrl4nav_amd.utils.recipe import make_weights
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": N, "int_frame_stack": C, "discrete_action": True,
           "discrete_actions": list(range(A)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg_nn = ConfigNN(env)
    cfg_nn.TRAINING_ITER_TIME = iters
    if share is not None:
        cfg_nn.SHARE_CNN_NET = share
    net = create_net({"config": BaseConfig(types.SimpleNamespace(task="device_env", ip="127.0.0.1"), env), "config_nn": cfg_nn,
                      "config_env": env}, max_batch=T * N)
    if share is None:
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_weights(seed, num_inputs=C, n_actions=A).items()})
    return net


def learn(net, ro):
    items = [({k: ld[k] for k in LOSS_KEYS}, ut) for ld, ut, _ in net.learn(ro.batch())]   # PpoBackUpTime is a wall clock
    assert items
    return items


LOSS_KEYS = ("PpoTotalLoss", "ActorLoss", "VLoss", "EntLoss")
POOLS = ("_actions", "_logps", "values", "_dones", "_rewards", "adv", "ret")


def snapshot(ro):
    torch.cuda.synchronize()
    return {k: getattr(ro, k).clone() for k in POOLS}


def test_closed_loop_equals_the_host_driven_rollout():
    """Variant A: PlaneRollout + DeviceEnv through collect(), frames rendered in the pool.  Variant B: DeviceRollout whose frames,
    rewards and dones come from the host model stepped with the actions read back.  Two rollouts with carry_over() between them."""
    from ddrl4nav_amd.agent import DeviceRollout, PlaneRollout
    from ddrl4nav_amd.env import DeviceEnv
    from ddrl4nav_amd.runner.device_loop import collect
    net_a, net_b = make_net(seed=3), make_net(seed=3)
    ra = PlaneRollout(net_a, N, horizon=T, channels=C, seed=11, track_returns=True)
    rb = DeviceRollout(net_b, N, horizon=T, channels=C, seed=11, track_returns=True)
    env = DeviceEnv("pong", N, device="cuda", **ENV_KW)
    model = R.DeviceEnvRef("pong", N, **ENV_KW)
    before = net_a.hot_path.params.clone()
    all_r, all_d = [], []
    for r in range(2):
        collect(ra, env)
        if r == 0:
            rb.put_new_frames(0, model.reset(), reset=True)
        for t in range(T):
            frame, reward, done = model.step(host(rb.act(t)))
            rb.record(t, reward, done)
            rb.put_new_frames(t + 1, frame)
            all_r.append(reward)
            all_d.append(done)
        rb.bootstrap()
        rb.finish()
        sa, sb = snapshot(ra), snapshot(rb)
        for k in POOLS:
            assert torch.equal(sa[k][:T], sb[k][:T]), (r, k)
        assert torch.equal(sa["values"], sb["values"]) and torch.equal(sa["_actions"], sb["_actions"])   # the bootstrap row too
        assert np.array_equal(host(ra.dones), np.stack(all_d[-T:])) and np.array_equal(host(ra.rewards), np.stack(all_r[-T:]))
        assert np.array_equal(host(env.state), model.state)
        for t in range(T + 1):                                          # the pool rows hold the model's frames
            assert torch.equal(ra.planes[ra.H + t], rb.frames[t][:, C - 1]), (r, t)
        items_a, items_b = learn(net_a, ra), learn(net_b, rb)
        assert items_a == items_b
        for k in ("params", "adam_m", "adam_v"):
            assert torch.equal(getattr(net_a.hot_path, k), getattr(net_b.hot_path, k)), (r, k)
        ra.carry_over()
        rb.carry_over()
    assert not torch.equal(net_a.hot_path.params, before)
    # ro.returns against the model's episode returns (Status.update_reward_status over the 2 T steps)
    rew, don = np.stack(all_r), np.stack(all_d)
    assert don[:T].sum() + don[T:].sum() >= N and don[T:].any()
    rsum, rep, fin = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32)
    for t in range(2 * T):
        rsum += rew[t]
        rep = np.where(don[t] != 0, rsum, rep)
        rsum = np.where(don[t] != 0, np.float32(0), rsum)
        fin += don[t] != 0
    for ro in (ra, rb):
        assert np.array_equal(host(ro.returns.rewards_episode), rep) and np.array_equal(host(ro.returns.episodes_finished), fin)
        assert np.array_equal(host(ro.returns.rewards_sum), rsum)
    assert ra.returns.mean_return() == float(rep[fin > 0].astype(np.float32).mean())


def test_in_pool_put_copies_nothing_and_a_foreign_frame_still_lands():
    """put_new_frames with the pool's own row skips the copy (the row keeps what the producer wrote, the age launch still runs); any
    other tensor is copied as before."""
    from ddrl4nav_amd.agent import PlaneRollout
    fake = types.SimpleNamespace(device=torch.device("cuda"), n_actions=A)
    ro = PlaneRollout(fake, N, horizon=T, channels=C)
    ro.age.fill_(77)
    row = ro.new_frame_row(0)
    assert row.data_ptr() == ro.planes[ro.H].data_ptr() and row.data_ptr() % 16 == 0 and tuple(row.shape) == (N, 84, 84)
    row.fill_(9)
    ro.put_new_frames(0, row, reset=True)
    assert bool((ro.planes[ro.H] == 9).all()) and bool((ro.age[0] == 0).all())
    other = torch.full((N, 84, 84), 5, dtype=torch.uint8, device="cuda")
    ro.put_new_frames(1, other, reset=False)
    assert bool((ro.planes[ro.H + 1] == 5).all()) and bool((ro.age[1] == 1).all())
    ro.put_new_frames(2, ro.new_frame_row(1), reset=False)              # another row of the pool is a source like any other
    assert bool((ro.planes[ro.H + 2] == 5).all())


def newest_frame(ro, t):
    """The single frame stored for slot t of either pool."""
    return ro.planes[ro.H + t] if hasattr(ro, "planes") else ro.frames[t][:, C - 1]


@pytest.mark.parametrize("pool", ["stacked", "planes", "planes_act_in_place"])
@pytest.mark.parametrize("keep_step", [False, True])
def test_collect_honours_both_carry_over_modes(keep_step, pool):
    """Three chained rollouts per mode and pool: the env's trajectory is the model's under the actions the rollouts stored, in order,
    with no step played twice or skipped (keep_step: the bootstrap action is played and its reward recorded in row T; its frame waits
    in env.frame and becomes slot 1 of the next rollout)."""
    from ddrl4nav_amd.agent import DeviceRollout, PlaneRollout
    from ddrl4nav_amd.env import DeviceEnv
    from ddrl4nav_amd.runner.device_loop import collect
    net = make_net(seed=5)
    if pool == "stacked":
        ro = DeviceRollout(net, N, horizon=T, channels=C, seed=2)
    else:
        ro = PlaneRollout(net, N, horizon=T, channels=C, seed=2, act_in_place=pool == "planes_act_in_place")
    env = DeviceEnv("catch", N, device="cuda", seed=13)
    model = R.DeviceEnvRef("catch", N, seed=13)
    frame = model.reset()
    for r in range(3):
        collect(ro, env, keep_step=keep_step)
        torch.cuda.synchronize()
        assert ro.t0 == (1 if keep_step and r > 0 else 0)
        acts, rew, don = host(ro._actions), host(ro._rewards), host(ro._dones)
        for t in range(ro.t0, T + 1 if keep_step else T):
            assert np.array_equal(host(newest_frame(ro, t)), frame), (r, t)
            frame, reward, done = model.step(acts[t])
            assert np.array_equal(rew[t], reward) and np.array_equal(don[t], done), (r, t)
        if not keep_step:
            assert np.array_equal(host(newest_frame(ro, T)), frame)
        assert np.array_equal(host(env.state), model.state)
        ro.carry_over(keep_step=keep_step)


@pytest.mark.parametrize("share", [False, True])
def test_train_runs_three_updates_on_catch(share):
    from ddrl4nav_amd.agent import PlaneRollout
    from ddrl4nav_amd.env import DeviceEnv
    from ddrl4nav_amd.runner.device_loop import train
    net = make_net(share=share, iters=2)
    ro = PlaneRollout(net, N, horizon=T, channels=C, seed=1, track_returns=True)
    env = DeviceEnv("catch", N, device="cuda", seed=4)
    start = net.update_time
    out = list(train(net, env, ro, 3))
    assert len(out) == 3 and net.update_time > start and ro.rollouts == 3
    for losses, mean_return in out:
        assert all(np.isfinite(losses[k]) for k in LOSS_KEYS)
        assert mean_return != mean_return or -1.0 <= mean_return <= 1.0
    assert -1.0 <= out[-1][1] <= 1.0                                    # 48 steps: every env has finished two episodes
