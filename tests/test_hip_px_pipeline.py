"""The chunk pipeline of the pair-exact convolutions (k_conv_px: conv_kernels.inc.h) where it can go wrong: a wave's list of
chunks shorter than the pipeline is deep, or ending inside a block of four.  The scenes below are built so that supertiles
execute exactly 1, 2, 3, 4, 5, 8, 9, 12, 13, 16 and 17 chunks in a time slice -- with four waves per supertile that is waves
with no block, one or two blocks and every remainder of a block; two time indices put chunks into all three segments (35 and
49 chunks: waves with three and four blocks) and start a second supertile, as does one scene of a single slice.

How a scene gets its count.  All voxels of a one-slice scene lie in one supertile (< 64 rows), and an offset holds a pair for
every two voxels that differ by it.  Level 1 pads an offset's pairs to 16: m isolated voxels and p two-voxel clusters, each
along another of the 13 directions, give ceil((m + 2 p) / 16) + 2 p chunks.  Level 0 pads to 8 pairs and packs two offsets
into a chunk: ceil((ceil((m + 2 p) / 8) + 2 p) / 2) chunks.  A scene for level 1 lives on the 0.2 m lattice, where its
level-0 voxels are all isolated.

The counts are computed on the CPU from the ORACLE's pair lists and the intended ones asserted before anything runs on the
GPU; there every scene is compared with the oracle (scores and tapped feature maps, tolerances of test_hip_parity), its chunk
counts are read back (rb_cnt through sps_get_rulebook_chunks), and a second run on the same context must repeat the first
bit for bit -- an operand set that survived into the next supertile or the next launch would not."""
import itertools
import os
import sys

import numpy as np
import pytest

from oracle import sps_oracle as O
from tests.helpers import CFG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

VS = CFG["MODEL"]["VOXEL_SIZE"]
WANTED = (1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17)
# the 13 directions of a 3x3x3 neighbourhood up to sign
DIRS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]
assert len(DIRS) == 13


def scene(m, p, scale, two_times=False):
    """m isolated voxels and p two-voxel clusters (cluster i along DIRS[i]) on the lattice of `scale` voxels, 8 lattice steps
    apart along x; [N, 6] float32 rows (b, x, y, z, t, label), one point per voxel, at the voxel centres."""
    ijk = [(8 * i, 0, 0) for i in range(m)]
    for i in range(p):
        base = (8 * (m + i), 4, 4)
        ijk += [base, tuple(b + d for b, d in zip(base, DIRS[i]))]
    ijk = np.asarray(ijk, np.int64) * scale
    xyz = (ijk.astype(np.float64) + 0.5) * VS
    out = np.zeros((len(ijk), 6), np.float32)
    out[:, 1:4] = xyz
    out[:, 4] = 1
    out[:, 5] = (np.arange(len(ijk)) % 5) / 4.0
    if two_times:
        again = out.copy()
        again[:, 4] = 0
        out = np.concatenate([out, again], 0)
    return out


def level0_scene(c, two_times=False):
    """c chunks in the dt = 0 segment of the level-0 supertile."""
    for p, m in itertools.product(range(14), range(0, 60)):
        if 0 < m + 2 * p < 64 and (-(-(m + 2 * p) // 8) + 2 * p + 1) // 2 == c:
            return scene(m, p, 1, two_times)
    raise AssertionError(c)


def level1_scene(c, two_times=False):
    """c chunks in the dt = 0 segment of the level-1 supertile."""
    for p, m in itertools.product(range(14), range(0, 60)):
        if 0 < m + 2 * p < 64 and -(-(m + 2 * p) // 16) + 2 * p == c:
            return scene(m, p, 2, two_times)
    raise AssertionError(c)


def scenes():
    out = {}
    for c in WANTED:
        out[f"level0_{c}"] = level0_scene(c)
        out[f"level1_{c}"] = level1_scene(c)
    out["level0_17_two_times"] = level0_scene(17, True)
    out["level1_17_two_times"] = level1_scene(17, True)
    # more than 64 rows at level 0: a second supertile starts (and ends after a few rows)
    out["two_supertiles"] = np.concatenate([scene(50, 9, 1), scene(3, 4, 1) + np.float32([0, 0, 3.0, 0, 0, 0])], 0)
    return out


def rows_of(want, got):
    """index into `got` of every row of `want` (the same coordinate set in two orders)."""
    assert want.shape == got.shape
    ow, og = np.lexsort(want.T[::-1]), np.lexsort(got.T[::-1])
    np.testing.assert_array_equal(want[ow], got[og])
    r = np.empty(len(want), np.int64)
    r[ow] = og
    return r


def chunks_from_oracle(batch, level):
    """[supertiles, 3] chunks per supertile and segment of the level's rulebook, from the oracle's pair lists: pairs padded
    to 16 per offset at level 1; to 8 at level 0, two such halves per chunk."""
    import granularity_stats as G
    vox, _ = O.unique_first(O.quantize(batch[:, :5], VS))
    cm = O.CoordinateManager(vox)
    ts = 1 << level
    if ts > 1:
        cm.ensure_stride(ts)
    oc = cm.coords[ts].copy()
    oc[:, 1:4] //= ts
    rows, _ = G.level_rows(batch, VS, levels=level + 1)
    dev_row = rows_of(oc, rows[level])
    nst = (len(oc) + 63) // 64
    n = np.zeros((nst, 81), np.int64)
    for k, (_, o) in enumerate(cm.k3(ts)):
        n[:, k] = np.bincount(dev_row[o] >> 6, minlength=nst)
    n = n.reshape(nst, 3, 27)
    if level == 0:
        return ((-(-n // 8)).sum(2) + 1) // 2
    return (-(-n // 16)).sum(2)


@pytest.fixture(scope="module")
def cases():
    """name -> (batch, chunks at level 0, chunks at level 1), with the intended counts asserted."""
    out = {name: (b, chunks_from_oracle(b, 0), chunks_from_oracle(b, 1)) for name, b in scenes().items()}
    for level in (0, 1):
        for c in WANTED:
            b, *ch = out[f"level{level}_{c}"]
            assert len(b) <= 300 and ch[level].tolist() == [[0, c, 0]], (level, c, ch[level].tolist())
        _, *ch = out[f"level{level}_17_two_times"]
        assert (ch[level][0] > 0).all() and ch[level][0].sum() > 32, ch[level]      # all three segments, > 8 blocks
    _, ch0, _ = out["two_supertiles"]
    assert len(ch0) == 2 and ch0[1].sum() > 0
    return out


def test_scenes_have_the_intended_chunk_counts(cases):
    """(no GPU) chunk counts per supertile of all scenes: 4 waves, blocks of four -- waves with 0 .. 4 blocks, and lists that
    end after 1, 2, 3 and 4 chunks of a block."""
    totals = sorted({int(t) for _, ch0, ch1 in cases.values() for ch in (ch0, ch1) for t in ch.sum(1)})
    assert set(WANTED) <= set(totals)
    assert {t % 4 for t in totals} == {0, 1, 2, 3}
    blocks_of_wave0 = {(-(-t // 4) + 3) // 4 for t in totals}
    assert {1, 2, 3, 4} <= blocks_of_wave0 and min(totals) < 4          # (1 block in all: three waves have none)


NAMES = sorted(scenes())


@pytest.fixture(scope="module")
def params():
    from sps_amd import synthetic
    from tests.helpers import straddle_params
    return straddle_params(O.random_params(seed=0), synthetic.small_scene(seed=11, n_scan=2500))


@pytest.fixture(scope="module")
def net(params):
    import torch
    from tests.helpers import net_from_params
    assert torch.cuda.is_available()
    return net_from_params(params).cuda().eval().freeze()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_short_chunk_lists(cases, net, params, name):
    import torch
    from tests import test_hip_parity as P
    batch, ch0, ch1 = cases[name]
    P.check_full(net, params, batch)                                   # scores, tapped feature maps, maps against the oracle
    c = P.ctx()
    np.testing.assert_array_equal(c.rulebook_chunks(0), ch0)
    np.testing.assert_array_equal(c.rulebook_chunks(1), ch1)
    taps = ("block1", "block7", "block8")
    _, s1 = P.run(net, batch)
    first = (s1.clone(), [P.get_feature(t) for t in taps])
    _, s2 = P.run(net, batch)
    assert torch.equal(first[0], s2) and bool(torch.isfinite(s2).all())
    for t, f in zip(taps, first[1]):
        np.testing.assert_array_equal(P.get_feature(t), f, err_msg=t)
