"""Host side of the scripted navigation expert (tests/nav_expert_ref.py, the rule book of csrc/navexpert.hip):
header, binding and exports, every refusal the operator decides before it touches HIP, the rule book's own claims (labels decode to the
chosen arc, keys below 2^22, every branch taken on a seeded set of states) and the expert's quality on the rule book's env."""
import itertools

import numpy as np
import pytest

import nav_env_ref as R
import nav_expert_ref as E
from arena_abi import header_declares

NEW = ("ddrl_op_nav_expert", "ddrl_op_heads_bc_mse_ws_floats", "ddrl_op_heads_bc_mse", "ddrl_op_gather_rows_f32")


def test_header_binding_and_exports():
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.env import NavExpert
    header_declares(NEW, [12, 3, 15, 7])                                    # additive: the ABI version stays 3
    assert all(callable(getattr(ops, k)) for k in ("nav_expert", "beta_threshold", "heads_bc_mse", "heads_bc_mse_ws_floats",
                                                    "gather_rows_f32"))
    assert callable(NavExpert.labels) and callable(NavExpert.mix)


def test_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses: every refusal below is decided before the first HIP call."""
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    a, M = 0x10000000, 0x1000000
    base = dict(st=a, pol=a + M, lab=a + 2 * M, pl=a + 3 * M)
    nbytes = dict(st=8 * 256, pol=8 * 8, lab=8 * 8, pl=8 * 8)      # at n = 8

    def expert(st=base["st"], n=8, env0=0, seed=1, nobs=10, nped=5, pol=base["pol"], step=3, thr=1 << 31, lab=base["lab"], pl=base["pl"]):
        return lib.ddrl_op_nav_expert(st, n, env0, seed, nobs, nped, pol, step, thr, lab, pl, None)

    bad = [dict(st=None), dict(pol=None, lab=None, pl=None), dict(n=0), dict(n=-3), dict(env0=-1), dict(env0=2 ** 32), dict(env0=2 ** 32 - 7),
           dict(nobs=-1), dict(nobs=11), dict(nped=-1), dict(nped=6), dict(st=a + 4), dict(st=a + 8), dict(pol=a + M + 2),
           dict(lab=a + 2 * M + 1), dict(pl=a + 3 * M + 2)]
    for p, q in itertools.permutations(("st", "pol", "lab", "pl"), 2):
        if q == "st":
            bad += [{q: base[p] - nbytes["st"] + 16}]                # the state's last 16 bytes on p's first
            continue
        bad += [{q: base[p]}, {q: base[p] + nbytes[p] - 4}]
    for kw in bad:
        assert expert(**kw) == -1, kw


def test_wrappers_refuse_what_they_cannot_take():
    import torch
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.env import FleetNavEnv, NavExpert
    with pytest.raises(AssertionError):
        ops.nav_expert(torch.zeros((4, 64), dtype=torch.int32), label=torch.zeros((4, 2)))          # host tensors
    for beta in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.beta_threshold(beta)
    with pytest.raises(NotImplementedError, match="FleetNavEnv"):
        NavExpert(FleetNavEnv.__new__(FleetNavEnv))
    with pytest.raises(TypeError):
        NavExpert(object())


def test_beta_threshold_arithmetic():
    from ddrl4nav_amd import ops
    for beta, want in ((0.0, 0), (1.0, 2 ** 32 - 1), (0.5, 2 ** 31), (0.25, 2 ** 30), (2.0 ** -32, 1), (1.0 - 2.0 ** -33, 2 ** 32 - 1),
                       (0.3, int(np.floor(0.3 * 2.0 ** 32)))):
        assert ops.beta_threshold(beta) == E.beta_threshold(beta) == want, beta
    # beta = 0 plays the policy everywhere, beta = 1 the expert unless the draw is the one value 2^32 - 1
    lab, pol = np.ones((64, 2), np.float32), np.zeros((64, 2), np.float32)
    assert not E.mix(lab, pol, 5, 0, 9, E.beta_threshold(0.0)).any() and E.mix(lab, pol, 5, 0, 9, E.beta_threshold(1.0)).all()
    half = E.expert_mask(4096, 5, 0, 9, E.beta_threshold(0.5)).mean()
    assert 0.45 < half < 0.55, half


# ---- the rule book's own claims -----------------------------------------------------------------------------------------------------------------
def test_candidates_and_labels_decode_to_the_chosen_arc():
    v, w = E.candidates()
    assert len(v) == 51 and sorted(set(v)) == [4, 16, 32] and sorted(set(w)) == list(range(-64, 65, 8))
    assert len({(a, b) for a, b in zip(v, w)}) == 51
    s = E.coverage_states()
    cv, cw = E.expert_choice(s, 10, 5)
    lab = E.expert_labels(s, 10, 5)
    assert lab.dtype == np.float32 and lab.shape == (len(s), 2)
    dv, dw = E.label_decodes(lab)
    assert np.array_equal(dv, cv) and np.array_equal(dw, cw)
    assert np.array_equal(lab[:, 0].astype(np.float64) * 32, cv) and np.array_equal(lab[:, 1].astype(np.float64) * 64, cw)    # exact


def test_every_branch_is_taken_and_keys_stay_below_2_22():
    """The model's own counts over the seeded states, as constants: a rule change shows here first."""
    c = {}
    key = E.expert_keys(E.coverage_states(), 10, 5, c)
    assert key.shape == (960, 51) and key.min() >= 0
    assert c["max_key"] == int(key.max()) < E.KEY_LIMIT
    # the bound by the rules: best <= 8191, bear <= 7,694, the diagonal of the +-2560 goal square against the +-(2560 + 320) pose square, ten steps of hit cost
    assert 64 * (8191 + (7694 >> 1) + 4096 * 10) + 50 < E.KEY_LIMIT
    want = {"arc_wall": 6753, "arc_obstacle": 1940, "arc_ped": 2341, "arc_free": 37926, "arrives": 197, "goal_behind": 13389,
            "key_tie": 29, "max_key": 3271376}
    assert c == want, c
    assert all(c[k] > 0 for k in E.BRANCHES)


def test_sanitised_like_the_step_kernel():
    """Random int32 words: the expert reads what NavEnvRef.sanitize leaves, and its input is not written."""
    rng = np.random.RandomState(5)
    raw = rng.randint(-2 ** 31, 2 ** 31, size=(16, 64), dtype=np.int64).astype(np.int32)
    keep = raw.copy()
    lab = E.expert_labels(raw, 3, 2)
    assert np.array_equal(raw, keep)
    m = R.NavEnvRef(16, n_obstacles=3, n_peds=2)
    m.state = raw.copy()
    m.sanitize()
    assert np.array_equal(E.expert_labels(m.state, 3, 2), lab)
    assert np.isin(lab[:, 0], [0.125, 0.5, 1.0]).all() and (np.abs(lab[:, 1]) <= 1).all()


# ---- the expert's quality on the rule book's env: N = 128, 500 steps, seed 3, max_steps = 300 ------------------------------------------------
# Measured with these rules (goals, obstacle hits, pedestrian hits, wall hits, truncations):
#   (10, 5)  733  13  48  0  0   reach rate 0.923        (3, 2)  925  2  14  0  0   reach rate 0.983        (0, 0)  996  0  0  0  0
@pytest.mark.parametrize("pop,floor", [((10, 5), 0.85), ((3, 2), 0.95), ((0, 0), 1.0)], ids=["10-5", "3-2", "0-0"])
def test_expert_reaches_its_goals(pop, floor):
    totals, _ = E.expert_tape(128, 500, 3, pop[0], pop[1], 300)
    rate = E.reach_rate(totals)
    print(pop, totals, "reach rate %.3f" % rate)
    assert totals["goal"] > 500
    assert rate >= floor, (pop, totals, rate)
    if pop == (0, 0):
        assert totals["obstacle_hit"] == totals["ped_hit"] == totals["wall_hit"] == totals["trunc"] == 0, totals
