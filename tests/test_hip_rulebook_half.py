"""GPU: the level-0 rulebook is padded per 8 pairs (half-chunks, two per chunk: map_kernels.inc.h) -- the chunk counts the
pair-exact convolutions execute, read back through rb_cnt, against bounds computed here from the exported pair sets."""
import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests.helpers import net_from_params, straddle_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net():
    assert torch.cuda.is_available()
    params = straddle_params(O.random_params(seed=0), synthetic.small_scene(seed=11, n_scan=2500))
    return net_from_params(params).cuda().eval().freeze()


def pairs_per_supertile(c, level):
    tab, n_entries = c.kernel_map(level, 1)                       # decoded from the rulebook itself
    pres = (tab.cpu().numpy() >= 0).T                             # [V, 81]
    assert int(pres.sum()) == n_entries
    V = len(pres)
    return np.pad(pres, ((0, (-V) % 64), (0, 0))).reshape(-1, 64, 3, 27).sum(1)   # [supertiles, slice, offset]


@pytest.mark.timeout(900)
def test_config2_level0_chunks_half_granular(net):
    """Config-2 scene: <= 136 500 chunks at level 0 (CPU model: 135 858; 154 511 under 16-pair padding), no supertile above
    its count under 16-pair padding, and every segment exactly ceil(halves / 2); level 1 keeps 16-pair chunks."""
    from sps_amd.models.models import get_context
    batch = synthetic.make_scene(scan_seed=1)["batch"]
    net(torch.from_numpy(np.ascontiguousarray(batch)).cuda())
    torch.cuda.synchronize()
    c = get_context(0)
    rb0 = c.rulebook_chunks(0)
    n0 = pairs_per_supertile(c, 0)
    assert rb0.shape == n0.shape[:2]
    bound16 = (-(-n0 // 16)).sum((1, 2))
    halves = (-(-n0 // 8)).sum(2)
    print(f"level 0: {int(n0.sum())} pairs, {int(rb0.sum())} chunks, {int(bound16.sum())} under 16-pair padding, "
          f"{int(((halves + 1) // 2).sum())} expected")
    assert int(rb0.sum()) <= 136_500
    assert (rb0.sum(1) <= bound16).all()
    np.testing.assert_array_equal(rb0, (halves + 1) // 2)
    rb1 = c.rulebook_chunks(1)
    n1 = pairs_per_supertile(c, 1)
    print(f"level 1: {int(n1.sum())} pairs, {int(rb1.sum())} chunks")
    np.testing.assert_array_equal(rb1, (-(-n1 // 16)).sum(2))
