"""The claims of tests/config_cross.py, and the yardstick of tests/test_config_cross_gpu.py on its own: in every cell the fp32 oracle's
gradient sits within HALF the bound the GPU test applies to the kernels (1e-5 max|g64| of 2e-5) and a tenth of its cosine allowance
(1 - 1e-10 of 1 - 1e-9) from the float64 oracle, both under the fp32 run's own leaky-ReLU decisions.  A cell where the fp32 reference
itself used up the bound could not tell a kernel fault from summation noise."""
import numpy as np
import pytest
import torch

import config_cross as X
from oracle import ddrl_oracle as O
import parity_util as P


def test_cells_are_a_pairwise_covering_array():
    assert X.uncovered_pairs(X.CELLS) == []
    assert len(X.CELLS) <= 16 and len(set(X.CELLS)) == len(X.CELLS)
    # the table helper must be able to fail: without its only (C = 4, A = 18) cell the pairs of that cell alone are reported
    assert ("C", 4, "A", 18) in X.uncovered_pairs([c for c in X.CELLS if (c.C, c.A) != (4, 18)])


def test_two_stacked_frames_meet_every_head_class_and_both_sharing_modes():
    two = [c for c in X.CELLS if c.C == 2]
    assert {c.A for c in two} == set(X.ACTIONS)
    assert {c.shared for c in two} == {0, 1}
    assert {c.shared for c in X.ACTING if c.C == 2} == {0, 1}


def test_every_cell_is_a_valid_config():
    for c in X.CELLS + X.ACTING:
        assert X.config_is_valid(c), c
        assert c.A in X.ACTIONS and c.C in X.CHANNELS
    for c in X.CELLS:
        assert c.n in X.BATCHES and c.max_batch in (c.n, 2 * c.n + 3) and c.n <= X.ACT_FUSED_MAX
    assert len(X.ACTING) <= 6
    for c in X.ACTING:
        assert c.n == c.max_batch == X.ACT_FUSED_MAX + 1 and c.C < 4
    assert {(c.C, c.shared) for c in X.ACTING} == {(C, s) for C in (1, 2, 3) for s in (0, 1)}
    seeds = [X.cell_seed(c) for c in X.CELLS + X.ACTING]
    assert len(set(seeds)) == len(seeds)


def test_cell_inputs_follow_the_recipe():
    c = X.CELLS[5]
    frames, acts, old, adv, ret, w = X.cell_inputs(c)
    again = X.cell_inputs(c)
    assert frames.shape == (c.n, c.C, 84, 84) and frames.dtype == np.uint8
    assert all(a.shape == (c.n,) and a.dtype == np.float32 for a in (acts, old, adv, ret))
    assert acts.min() >= 0 and acts.max() <= c.A - 1 and np.array_equal(acts, np.floor(acts))
    assert np.array_equal(frames, again[0]) and all(np.array_equal(a, b) for a, b in zip((acts, old, adv, ret), again[1:5]))
    assert w["actor.pre.conv1.weight"].shape == (32, c.C, 8, 8) and w["actor.actor_linear.weight"].shape == (c.A, 512)
    assert "prenet.conv1.weight" in X.cell_inputs(X.CELLS[1])[5]


@pytest.mark.parametrize("cell", X.CELLS, ids=X.cell_id)
def test_fp32_oracle_is_inside_half_the_gpu_bound(cell):
    frames, acts, old, adv, ret, w = X.cell_inputs(cell)
    cls = O.OracleSharedPPO if cell.shared else O.OraclePPO
    x = O.frames_to_f32(frames)
    t = torch.from_numpy
    threads = torch.get_num_threads()
    torch.set_num_threads(P.oracle_threads())
    try:
        nets = []
        for dtype in (torch.float32, torch.float64):
            net = cls(n_actions=cell.A, num_inputs=cell.C)
            net.load_weights(w)
            nets.append(net.to(dtype))
        net32, net64 = nets
        with torch.no_grad():
            net32(x)
        for a, b in zip((m for m in net32.modules() if isinstance(m, O.Encoder)), (m for m in net64.modules() if isinstance(m, O.Encoder))):
            a.forced = b.forced = [z > 0 for z in a.last_z]
        P.ppo_backward(net32, x, t(acts), t(old), t(adv), t(ret), bool(cell.smooth_l1))
        P.ppo_backward(net64, x.double(), t(acts).double(), t(old).double(), t(adv).double(), t(ret).double(), bool(cell.smooth_l1))
    finally:
        torch.set_num_threads(threads)
    worst = (0.0, 0.0, "")
    for (name, p32), (_, p64) in zip(net32.named_parameters(), net64.named_parameters()):
        g32, g64 = p32.grad.double().numpy().ravel(), p64.grad.numpy().ravel()
        scale = np.abs(g64).max()
        assert scale > 0, name
        err = np.abs(g32 - g64).max() / scale
        one_minus_cos = 1.0 - g32 @ g64 / (np.linalg.norm(g32) * np.linalg.norm(g64))
        worst = max(worst, (err, one_minus_cos, name))
        assert err <= 1e-5, (name, err)
        assert one_minus_cos < 1e-10, (name, one_minus_cos)
    print("%s: fp32 oracle against float64, worst tensor %s: %.2e max|g64|, 1 - cos %.1e" % (X.cell_id(cell), worst[2], worst[0], worst[1]))
