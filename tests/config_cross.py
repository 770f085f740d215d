"""Cell tables of tests/test_config_cross_gpu.py: the configuration knobs of the fused Atari context (ddrl_config: in_channels, n_actions,
share_cnn_net, smooth_l1_loss, max_batch) crossed with the batch size, and the inputs of a cell.  No GPU: the tables can be inspected (and their
own claims checked, tests/test_config_cross_cpu.py) anywhere."""
from collections import namedtuple

import numpy as np

# ---- factor levels ---------------------------------------------------------------------------------------------------------------------
CHANNELS = [1, 2, 3, 4]     # in_channels: run-time C of the conv1 packer (optim.hip), the fused acting kernel (act.hip), the two conv1 forwards
                            # (conv2.hip) and the conv1 weight gradient (wgrad2.hip: ktaps = 64 C, partial slab 32 * 64 C + 32)
ACTIONS = [
    2,      # A <= 6: heads_loss_kernel<6, ...>, the four samples' dot products reduced together, gradients in registers; the smallest A
    7,      # 7..8:   heads_loss_kernel<8, false>: head weights in registers, per-sample reduction, one padded action row
    9,      # > 8:    heads_loss_kernel<18, true> (weights in LDS) + head_wgrad_kernel; heads_act_kernel<18, true>; nine padded rows
    18,     # > 8:    the same kernels with no padded row (the full Atari action set, the ABI's maximum)
]
SHARED = [0, 1]             # share_cnn_net: NE = 2 or 1 in every encoder kernel (ROWS = 32 NE, enc_base[NE - 1], split counts x NE)
SMOOTH_L1 = [0, 1]          # smooth_l1_loss: the branch of the value loss
BATCHES = [
    1,      # a single sample: every tile, pair and k-block ragged
    37,     # an odd sample pair, 12 conv2 tiles of 3 + 1 sample, 7 conv3 tiles of 5 + 2 samples, one 32-sample k-block + 5
    131,    # four 32-sample k-blocks + 3, a last conv2 tile of two samples, a last conv3 tile of one, an odd pair
]
ROOMY = [0, 1]              # capacity: max_batch = n (the ragged tail ends every workspace tensor and the caller's frame buffer), or
                            # max_batch = 2 n + 3 (strides differ from n; choose_splits(max_batch) gives more splits than sample pairs: empty slabs)

Cell = namedtuple("Cell", "C A shared smooth_l1 n max_batch")


def capacity(n, roomy):
    return 2 * n + 3 if roomy else n


def _cell(C, A, shared, smooth_l1, n, roomy):
    return Cell(C, A, shared, smooth_l1, n, capacity(n, roomy))


# A pairwise covering array over the six factors above: all 16 (C, A) pairs once; shared, smooth_l1 and the capacity are parities of the two
# indices (shared = (i ^ j) & 1, smooth_l1 = ((i ^ j) >> 1) & 1, roomy = (i ^ (j >> 1)) & 1 with i, j the positions of C and A), n was placed
# by search.  tests/test_config_cross_cpu.py checks the cover by enumeration.  C = 2 -- which no other test runs through the encoder -- meets
# every A class and both sharing modes.
CELLS = [
    #     C   A  shared smooth  n  roomy
    _cell(1,  2, 0, 0,   1, 0),
    _cell(1,  7, 1, 0, 131, 0),
    _cell(1,  9, 0, 1,   1, 1),
    _cell(1, 18, 1, 1,  37, 1),
    _cell(2,  2, 1, 0, 131, 1),
    _cell(2,  7, 0, 0,  37, 1),
    _cell(2,  9, 1, 1,  37, 0),
    _cell(2, 18, 0, 1,   1, 0),
    _cell(3,  2, 0, 1,  37, 0),
    _cell(3,  7, 1, 1,   1, 0),
    _cell(3,  9, 0, 0, 131, 1),
    _cell(3, 18, 1, 0, 131, 1),
    _cell(4,  2, 1, 1,  37, 1),
    _cell(4,  7, 0, 1, 131, 1),
    _cell(4,  9, 1, 0,   1, 0),
    _cell(4, 18, 0, 0,  37, 0),
]

# The batch-tiled acting forward (n > ACT_FUSED_MAX = 512) for the frame stacks below four, both sharing modes; each C meets both forms of
# heads_act_kernel (A <= 8: register weights, one wave per workgroup; A > 8: LDS weights, four waves).  smooth_l1 plays no part in a forward.
ACT_FUSED_MAX = 512
ACTING = [
    Cell(1,  2, 0, 0, 513, 513),
    Cell(1, 18, 1, 0, 513, 513),
    Cell(2,  9, 0, 0, 513, 513),
    Cell(2,  7, 1, 0, 513, 513),
    Cell(3, 18, 0, 0, 513, 513),
    Cell(3,  2, 1, 0, 513, 513),
]

FACTORS = [("C", CHANNELS), ("A", ACTIONS), ("shared", SHARED), ("smooth_l1", SMOOTH_L1), ("n", BATCHES), ("roomy", ROOMY)]


def levels(cell):
    """The cell's level of every factor of FACTORS, in that order."""
    assert cell.max_batch in (cell.n, 2 * cell.n + 3)
    return (cell.C, cell.A, cell.shared, cell.smooth_l1, cell.n, int(cell.max_batch != cell.n))


def uncovered_pairs(cells):
    """[(factor a, level, factor b, level)] that no cell holds: empty for a pairwise covering array."""
    have = [levels(c) for c in cells]
    missing = []
    for a in range(len(FACTORS)):
        for b in range(a + 1, len(FACTORS)):
            seen = {(lv[a], lv[b]) for lv in have}
            missing += [(FACTORS[a][0], x, FACTORS[b][0], y) for x in FACTORS[a][1] for y in FACTORS[b][1] if (x, y) not in seen]
    return missing


def config_is_valid(cell):
    """validate() of csrc/api.hip for the fields a cell sets."""
    return (cell.max_batch >= 1 and 2 <= cell.A <= 18 and 1 <= cell.C <= 4 and cell.shared in (0, 1)
            and cell.max_batch * 32 * 400 * 4 < 1 << 32 and 1 <= cell.n <= cell.max_batch)


def cell_id(cell):
    return "C%d-A%d-%s-%s-n%d-mb%d" % (cell.C, cell.A, "shared" if cell.shared else "split", "smoothl1" if cell.smooth_l1 else "mse", cell.n, cell.max_batch)


def cell_seed(cell):
    """One seed per cell, from its own fields (mixed radix: no two cells of the tables share one)."""
    return ((((cell.C * 19 + cell.A) * 2 + cell.shared) * 2 + cell.smooth_l1) * 1024 + cell.n) * 2048 + cell.max_batch


def cell_inputs(cell):
    """(frames u8 [n, C, 84, 84], actions, old_logps, advs, rets, weights) of a cell: uniform random bytes, actions uniform in 0..A-1,
    old_logps = -log A + N(0, 0.3), advantages and returns N(0, 1), weights from the recipe -- as test_gpu_parity.test_action_counts_vs_oracle."""
    from ddrl4nav_amd.utils.recipe import make_weights
    seed = cell_seed(cell)
    rng = np.random.default_rng(seed)
    n, A = cell.n, cell.A
    frames = rng.integers(0, 256, size=(n, cell.C, 84, 84), dtype=np.uint8)
    acts = rng.integers(0, A, size=n).astype(np.float32)
    old = (np.full(n, -np.log(A)) + rng.normal(0, 0.3, n)).astype(np.float32)
    adv = rng.normal(size=n).astype(np.float32)
    ret = rng.normal(size=n).astype(np.float32)
    w = make_weights(seed, num_inputs=cell.C, n_actions=A, shared=bool(cell.shared))
    return frames, acts, old, adv, ret, w
