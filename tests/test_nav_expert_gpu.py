"""csrc/navexpert.hip against its rule book (tests/nav_expert_ref.py): labels and played actions equal the
model's bit for bit -- over tapes the expert itself drives at N = 1, 5 and 67 (a last workgroup with three idle waves) under five
populations, at the top of the 32-bit env indices, under three mixing rates and two seeds, on random int32 words, into rows of a larger
buffer -- and the env's state is never written."""
import functools

import numpy as np
import pytest
import torch

import nav_expert_ref as E

pytestmark = pytest.mark.gpu

STEPS = 40
POPULATIONS = [(10, 5), (0, 0), (10, 0), (0, 5), (3, 2)]


@functools.lru_cache(maxsize=None)
def ref_tape(n, pop, seed, env0):
    """The rule book's expert tape: ([state before step t], [label t])."""
    _, tape = E.expert_tape(n, STEPS, seed, pop[0], pop[1], 60, env0=env0, record=True)
    return [s for s, _ in tape], [a for _, a in tape]


def device_pair(n, pop, seed, env0):
    from ddrl4nav_amd.env import DeviceNavEnv, NavExpert
    env = DeviceNavEnv(n, seed=seed, n_obstacles=pop[0], n_peds=pop[1], max_steps=60, env0=env0)
    env.reset()
    return env, NavExpert(env)


@pytest.mark.parametrize("pop", POPULATIONS, ids=lambda p: "%d-%d" % p)
@pytest.mark.parametrize("n", [1, 5, 67])
def test_expert_drives_the_env_as_the_rule_book(n, pop):
    env, expert = device_pair(n, pop, 9, 0)
    states, labels = ref_tape(n, pop, 9, 0)
    got = torch.empty((STEPS, n, 2), dtype=torch.float32, device=env.device)
    seen = torch.empty((STEPS, n, 64), dtype=torch.int32, device=env.device)
    for t in range(STEPS):
        seen[t].copy_(env.state)
        env.step(expert.labels(out=got[t]))
    assert np.array_equal(seen.cpu().numpy(), np.stack(states))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), np.stack(labels).view(np.uint32))


def test_top_of_the_env_indices():
    n, pop, env0 = 67, (10, 5), 2 ** 32 - 67
    env, expert = device_pair(n, pop, 4, env0)
    states, labels = ref_tape(n, pop, 4, env0)
    rng = np.random.RandomState(1)
    for t in range(12):
        assert np.array_equal(env.state.cpu().numpy(), states[t])
        policy = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        lab, played = expert.mix(torch.from_numpy(policy).to(env.device), 0.5, t)
        assert np.array_equal(lab.cpu().numpy(), labels[t])
        want = E.mix(labels[t], policy, 4, env0, t, E.beta_threshold(0.5))
        assert np.array_equal(played.cpu().numpy().view(np.uint32), want.view(np.uint32))
        env.step(lab)


@pytest.mark.parametrize("seed", [3, 0xDEADBEEF])
@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
def test_mixing_is_the_rule(beta, seed):
    n, pop = 67, (3, 2)
    env, expert = device_pair(n, pop, seed, 100)
    states, labels = ref_tape(n, pop, seed, 100)
    rng = np.random.RandomState(2)
    taken = 0
    for t in (0, 1, 7, 2 ** 32 - 1):
        policy = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        policy[0] = (np.nan, -0.0)                                   # bits are copied, not values
        lab, played = expert.mix(torch.from_numpy(policy).to(env.device), beta, t)
        assert np.array_equal(lab.cpu().numpy(), labels[0])
        mask = E.expert_mask(n, seed, 100, t, E.beta_threshold(beta))
        taken += int(mask.sum())
        want = E.mix(labels[0], policy, seed, 100, t, E.beta_threshold(beta))
        assert np.array_equal(played.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(env.state.cpu().numpy(), states[0])
    assert taken == {0.0: 0, 1.0: 4 * n}.get(beta, taken) and (beta != 0.5 or 0 < taken < 4 * n)


def test_random_words_are_sanitised():
    from ddrl4nav_amd import ops
    rng = np.random.RandomState(5)
    raw = rng.randint(-2 ** 31, 2 ** 31, size=(9, 64), dtype=np.int64).astype(np.int32)
    st = torch.from_numpy(raw).cuda()
    lab = torch.empty((9, 2), dtype=torch.float32, device="cuda")
    for pop in ((3, 2), (10, 5), (0, 0)):
        ops.nav_expert(st, label=lab, n_obstacles=pop[0], n_peds=pop[1])
        assert np.array_equal(lab.cpu().numpy(), E.expert_labels(raw, *pop)), pop
    assert np.array_equal(st.cpu().numpy(), raw)


def test_outputs_land_in_their_rows_only_and_repeat():
    n, pop = 5, (10, 5)
    env, expert = device_pair(n, pop, 9, 0)
    _, labels = ref_tape(n, pop, 9, 0)
    guard = float.fromhex("0x1.234p5")
    big_l = torch.full((3 * n, 2), guard, dtype=torch.float32, device=env.device)
    big_p = torch.full((3 * n, 2), guard, dtype=torch.float32, device=env.device)
    policy = torch.full((n, 2), 0.25, dtype=torch.float32, device=env.device)
    before = env.state.clone()
    expert.mix(policy, 0.5, 3, labels_out=big_l[n:2 * n], played_out=big_p[n:2 * n])
    first = (big_l.clone(), big_p.clone())
    expert.mix(policy, 0.5, 3, labels_out=big_l[n:2 * n], played_out=big_p[n:2 * n])
    assert torch.equal(first[0], big_l) and torch.equal(first[1], big_p)                       # a repeat is bit-identical
    assert torch.equal(env.state, before)                                                      # the expert only reads the env
    for big in (big_l, big_p):
        assert bool((big[:n] == guard).all()) and bool((big[2 * n:] == guard).all())
    assert np.array_equal(big_l[n:2 * n].cpu().numpy(), labels[0])
    want = E.mix(labels[0], policy.cpu().numpy(), 9, 0, 3, E.beta_threshold(0.5))
    assert np.array_equal(big_p[n:2 * n].cpu().numpy(), want)
    # labels alone, played alone
    only = torch.full((n, 2), guard, dtype=torch.float32, device=env.device)
    assert np.array_equal(expert.labels(out=only).cpu().numpy(), labels[0])
    from ddrl4nav_amd import ops
    ops.nav_expert(env.state, played=only, policy=policy, step=3, threshold=E.beta_threshold(0.5), env0=0, seed=9, n_obstacles=10, n_peds=5)
    assert np.array_equal(only.cpu().numpy(), want)
