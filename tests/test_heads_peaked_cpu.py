"""The peaked recipe of tests/test_heads_peaked_gpu.py where no GPU is needed: heads_ref.check_peaked_recipe on every case of the GPU grids
(every clamp decision at a stated distance in float64, torch's own float32 forward on the same side of each), the float64 reference's
exact zeros, the boundary cases, and the float64 statement of the collapse loop with the threshold the GPU loop is held to."""
import math

import pytest
import torch

import heads_peaked_ref as R
import heads_ref as H
import loss_options_ref as LR

GRID, OPT_GRID = R.grid(), R.opt_grid()


def test_grids_cover_what_they_say():
    assert len(GRID) == 20 and len(set(GRID)) == 20 and len(set(OPT_GRID)) == len(OPT_GRID)
    main = [s for s in GRID if s[4] == "main"]
    assert {(s[0], s[1]) for s in main} == {(A, n) for A in R.SIZES for n in R.BATCHES}
    for A in R.SIZES:
        assert {s[2] for s in main if s[0] == A} == {0, 1} and {s[3] for s in main if s[0] == A} == {0, 1}
        assert {s[2] for s in GRID if s[0] == A and s[4] == "underflow"} == {0, 1}
        mine = [s for s in OPT_GRID if s[0] == A]
        assert {s[6] for s in mine} == {"entropy", "both"} and {s[4] for s in mine} == {"main", "underflow"}
        assert any(s[2] == 0 and s[6] == "entropy" for s in mine)       # split encoders under the split entropy bonus
    # the five classes of gaps
    for A in (2, 3, 5, 6, 7):
        assert not any(15.0 < g < 17.5 for g in H.peaked_gaps(A))       # class (c) does not exist below A = 8
    for A in (8, 9, 13, 18):
        assert 16.2 in H.peaked_gaps(A)
    for A in R.SIZES:
        gaps = H.peaked_gaps(A)
        assert {0.0, 3.0} <= set(gaps) and {9.0, 13.0} <= set(gaps) and {20.5, 30.0, 40.0} <= set(gaps)


@pytest.mark.parametrize("spec", GRID + OPT_GRID, ids=R.case_id)
def test_peaked_recipe_keeps_its_margins(spec):
    c = R.case_of(spec)
    H.check_peaked_recipe(c)
    if len(spec) > 6 and c.value_clip > 0:
        LR.check_clip_recipe(c)
    tol = R.row_tol(c)
    zmax = c.z64.abs().amax(1)
    assert bool((tol[zmax < 4.0] <= 1.1 * R.OP_TOL).all()) and float(tol.max()) <= (8.2e-5 if spec[4] == "underflow" else 5.1e-5)
    assert bool((tol >= R.OP_TOL).all())


def test_recipe_conditions_hold_for_every_head_size():
    """The fp32 / float64 agreement over the sizes and gaps the recipe was worked out on -- and fails where it must: A = 2 at gap 16.2 has
    its one tail entry 0.26 from eps."""
    for A in (2, 3, 5, 6, 7, 8, 9, 13, 18):
        for gaps in (None, H.UNDERFLOW_GAPS):
            H.check_peaked_recipe(H.make_peaked_case(A, 257, A % 2, 1, seed=2, gaps=gaps))
    with pytest.raises(AssertionError):
        H.check_peaked_recipe(H.make_peaked_case(2, 257, 0, 0, seed=2, gaps=(16.2, 0.0, 30.0)))


def test_float64_rows_vanish_exactly_where_both_clamps_are_shut():
    """Split encoders without the entropy option: a row's float64 actor gradient is exactly 0 where the surrogate is flat OR the taken
    action's probability is outside [eps, 1 - eps]; torch's float32 run has its zeros in the same rows.  With the entropy option no row
    of a main case is exactly 0 (log(clamp(q_j)) itself has a gradient through q_j's weight in the sum)."""
    for spec in ((6, 257, 0, 0, "main", 257), (18, 67, 0, 1, "main", 67), (8, 67, 0, 0, "underflow", 67)):
        c = R.case_of(spec)
        r64, r32 = H.loss_block(c, torch.float64), H.loss_block(c, torch.float32)
        q = torch.softmax(c.z64, -1).gather(1, c.actions.long()[:, None])[:, 0]
        shut = (q < H.CAT_EPS) | (q > 1.0 - H.CAT_EPS)
        flat = torch.tensor([o in ("zero", "neg_dual", "pos_above", "neg_below") for o in c.outcomes])
        dead = r64["dh_actor"].abs().amax(1) == 0
        assert torch.equal(dead, shut | flat) and bool((shut & ~flat).any())
        assert torch.equal(r32["dh_actor"].abs().amax(1) == 0, dead)
        if spec[4] == "underflow":
            assert bool(dead.all())
    c = R.case_of((6, 257, 0, 0, "main", 257, "entropy"))
    assert bool((LR.loss_block(c, torch.float64)["dh_actor"].abs().amax(1) > 0).all())


def test_boundary_cases_sit_on_the_closed_boundary_in_float32_and_inside_in_float64():
    assert 15.8 < R.BOUNDARY_GAP < 15.85
    for A in R.SIZES:
        for shared in (0, 1):
            c = R.make_boundary_case(A, 9, shared)
            R.check_boundary_case(c)
            # what opening the interval would do to the float64 rows: the rows that took `top` lose their whole actor gradient, and
            # the entropy rows move by more than twice the bound they are held to
            c.entropy_split, c.value_clip = True, 0.0
            r = LR.loss_block(c, torch.float64)
            if not shared:
                assert bool((r["dh_actor"].abs().amax(1) > 0).all())


def test_float64_collapse_loop_stays_finite_and_ends_far_below_the_threshold():
    c = R.collapse_case()
    assert not c.shared and c.entropy_split and c.value_clip == 0 and c.hyper["ent_loss_theta"] == 0.01
    stats, params = R.collapse_loop64(c)
    assert stats.shape == (R.COLLAPSE_STEPS, 3) and bool(torch.isfinite(stats).all())
    assert all(bool(torch.isfinite(p).all()) for p in params.values())
    ent = stats[:, 2]
    print("float64 entropy: first %.4f, step 6 %.3e, last %.3e" % (float(ent[0]), float(ent[5]), float(ent[-1])))
    assert 1.0 < float(ent[0]) < math.log(R.COLLAPSE_A)
    assert float(ent[-1]) <= R.H_END / 10.0 and float(ent[-100:].max()) <= R.H_END / 10.0
    z = c.ha.double() @ params["actor_w"].T + params["actor_b"]
    assert bool((z.argmax(1) == R.FAVOURED).all())
