"""conv_dgrad3_planes_kernel orders its 243 tile columns (output row, sample, x) and does not issue the (column tile, tap) products
whose tap row only reads the zero border (conv2.hip Dgrad3Rows).  What can go wrong with that is local: a tap lost at one output
row, a column mapped to the wrong (sample, pixel), a tail sample stored or dropped.  So dz2 is compared against float64 PER OUTPUT
POSITION (y, x), at the batch sizes that leave a lone partial tile (n = 1, 2), a full tile (3), tails of one and two samples behind
full tiles (4, 5, 7) and pad columns next to real ones in the last column tile (every n).  Random dense inputs make every
(pixel, tap) term non-zero, so a wrongly skipped product is an O(1) relative error at the positions it feeds, not a rounding one."""
import numpy as np
import pytest
import torch

import parity_util as P
from test_gpu_parity import KINDS, _bwd_setup, _leaky_mask, hp  # noqa: F401  (hp: the module's HotPath fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_conv3_data_gradient_every_output_position(hp, kind, n):  # noqa: F811
    """Given the kernel's own dz3 and a2: dz2 = leaky'(a2) * conv_transpose(dz3, W3) against float64, the maximum error of each of
    the 81 output positions separately under the bound test_conv3_data_gradient_is_at_least_fp32_accurate applies to the tensor's
    maximum: conv3_dgrad_units rounding units (2^-24) of the largest sum |dz3 W3|."""
    w = _bwd_setup(hp, n, 4200 + n, kind)
    limit = P.MARGINS.limit("accuracy", "conv3_dgrad_units")
    ct = torch.nn.functional.conv_transpose2d
    bad = []
    for enc, pre in ((0, "actor.pre"), (1, "critic.pre")):
        dz3 = hp.debug_buffer(6, (64, 7, 7), n, enc).cpu()
        a2 = hp.debug_buffer(1, (64, 9, 9), n, enc).cpu()
        dz2 = hp.debug_buffer(5, (64, 9, 9), n, enc).cpu().numpy().astype(np.float64)
        W = torch.from_numpy(w[pre + ".conv3.weight"])
        ref = _leaky_mask(a2.double(), ct(dz3.double(), W.double())).numpy()
        assert dz2.shape == ref.shape == (n, 64, 9, 9)
        assert (np.abs(ref).max(axis=(0, 1)) > 0).all()  # no position is trivially zero
        mass = float(ct(dz3.double().abs(), W.double().abs()).max())
        units = np.abs(dz2 - ref).max(axis=(0, 1)) / (2.0 ** -24 * mass)  # [9, 9]: worst sample and channel of every position
        print("%s %s n=%d: worst position %.3f units of %.1f" % (kind, pre, n, units.max(), limit))
        bad += ["%s (y=%d, x=%d): %.4g units" % (pre, y, x, units[y, x]) for y in range(9) for x in range(9) if not units[y, x] <= limit]
    assert not bad, "dz2 positions beyond %.1f rounding units (%s, n=%d): %s" % (limit, kind, n, "; ".join(bad))
