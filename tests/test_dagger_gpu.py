"""The closed DAgger loop on the device (ddrl4nav_amd/runner/dagger_loop.py, data/demo_pool.py) against the
rule books: with beta = 1 the pool is the expert's own tape (observations through NavEnvRef.observe, labels through nav_expert_ref),
with beta = 0.5 the played actions are the rule's selection, the ring wraps where the arithmetic says, two runs from the same seeds end
in the same bits, and on one fixed pool the clone loss goes down."""
import numpy as np
import pytest
import torch

import generic_cross as X
import nav_env_ref as R
import nav_expert_ref as E

pytestmark = pytest.mark.gpu

N, POP, SLOTS, STEPS, SEED, MAX_STEPS = 8, (3, 2), 24, 16, 21, 40
CELL = X.Cell("nav1d_split", "gauss2", 0, "default", "none", 0, 2, 64)


def build(torch_seed=5):
    import test_generic_cross_gpu as GX
    from ddrl4nav_amd.data import DemoPool
    from ddrl4nav_amd.env import DeviceNavEnv, NavExpert
    torch.manual_seed(torch_seed)
    net = GX.make_net(CELL)
    assert net.continuous and net.n_actions == 2 and net.cap == 64
    env = DeviceNavEnv(N, seed=SEED, n_obstacles=POP[0], n_peds=POP[1], max_steps=MAX_STEPS)
    env.reset()
    pool = DemoPool(env.state_shapes, 2, N * SLOTS, device=env.device, n_envs=N)
    return net, env, NavExpert(env), pool


def ref_env():
    m = R.NavEnvRef(N, seed=SEED, n_obstacles=POP[0], n_peds=POP[1], max_steps=MAX_STEPS)
    return m, m.reset()


def assert_rows(pool, t, obs, labels=None):
    comps, lab = pool.rows(t)
    for name, got, want in zip(("laser", "vector", "image"), comps, obs):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (t, name)
    if labels is not None:
        assert np.array_equal(lab.cpu().numpy().view(np.uint32), labels.view(np.uint32)), (t, "labels")


def test_beta_one_fills_the_pool_with_the_experts_tape_and_wraps():
    from ddrl4nav_amd.runner import dagger_loop as L
    net, env, expert, pool = build()
    m, obs = ref_env()
    tape = []                                                          # (observation, label) of row set t
    for t in range(2 * STEPS + 1):
        lab = E.expert_labels(m.state, *POP)
        tape.append((obs, lab))
        obs = m.step(lab)[0]
    assert L.collect(net, env, expert, pool, STEPS, 1.0) == STEPS
    assert pool.cursor == STEPS + 1 and pool.pending and pool.labelled_rows().tolist() == list(range(N * STEPS))
    for t in range(STEPS):
        assert_rows(pool, t, *tape[t])
    assert_rows(pool, STEPS, tape[STEPS][0])                           # rendered, waiting for its label
    assert np.array_equal(env.state.cpu().numpy(), _state_after(STEPS))
    # ---- a second collect labels the waiting set first and wraps: sets 24 .. 32 lie over 0 .. 8
    assert L.collect(net, env, expert, pool, STEPS, 1.0, step0=STEPS) == 2 * STEPS
    assert pool.cursor == 2 * STEPS + 1 and pool.pending
    for slot in range(SLOTS):
        t = slot + SLOTS if slot + SLOTS <= 2 * STEPS else slot
        assert_rows(pool, t, tape[t][0], tape[t][1] if t < 2 * STEPS else None)
    waiting = 2 * STEPS % SLOTS
    assert pool.labelled_rows().tolist() == [r for r in range(N * SLOTS) if r // N != waiting]
    # ---- close=True: the last observation goes to the env's own tensors and no row waits
    L.collect(net, env, expert, pool, 2, 1.0, step0=2 * STEPS, close=True)
    assert not pool.pending and pool.cursor == 2 * STEPS + 2 and len(pool) == N * SLOTS


def _state_after(steps):
    m, _ = ref_env()
    for _ in range(steps):
        m.step(E.expert_labels(m.state, *POP))
    return m.state


def test_beta_half_plays_the_rules_selection():
    from ddrl4nav_amd.runner import dagger_loop as L
    net, env, expert, pool = build()
    record = []
    L.collect(net, env, expert, pool, STEPS, 0.5, step0=7, record=record)
    m, obs = ref_env()
    from_expert = 0
    for t, (policy, played) in enumerate(record):
        lab = E.expert_labels(m.state, *POP)
        assert_rows(pool, t, obs, lab)
        policy, played = policy.cpu().numpy(), played.cpu().numpy()
        want = E.mix(lab, policy, SEED, 0, 7 + t, E.beta_threshold(0.5))
        assert np.array_equal(played.view(np.uint32), want.view(np.uint32)), t
        from_expert += int(E.expert_mask(N, SEED, 0, 7 + t, E.beta_threshold(0.5)).sum())
        obs = m.step(played)[0]
    assert 0 < from_expert < N * STEPS
    assert np.array_equal(env.state.cpu().numpy(), m.state)


def test_two_runs_from_the_same_seeds_end_in_the_same_bits():
    from ddrl4nav_amd.runner import dagger_loop as L
    ends = []
    for _ in range(2):
        net, env, expert, pool = build(torch_seed=9)
        out = list(L.run(net, env, expert, pool, iterations=2, steps=6, lr=3e-4, batch=32, epochs=2, seed=3))
        assert [b for _, b in out] == [1.0, 0.0] and all(np.isfinite(l) for l, _ in out)
        ends.append((net.params.clone(), pool.labels.clone(), env.state.clone(), out))
    assert torch.equal(ends[0][0].view(torch.int32), ends[1][0].view(torch.int32))
    assert torch.equal(ends[0][1], ends[1][1]) and torch.equal(ends[0][2], ends[1][2]) and ends[0][3] == ends[1][3]


def test_clone_loss_goes_down_on_a_fixed_pool():
    """A fitting check on fixed data, the only learning claim a test makes: every step sees the same 128 rows."""
    from ddrl4nav_amd.runner import dagger_loop as L
    net, env, expert, pool = build()
    L.collect(net, env, expert, pool, STEPS, 1.0)
    log = net.clone_actor(pool, 3e-4, N * STEPS, 30, seed=1)
    losses = [row[2] for row in log]
    print("clone loss, step 1: %.6g, step 30: %.6g" % (losses[0], losses[29]))
    assert len(losses) == 30 and losses[29] < losses[0]
