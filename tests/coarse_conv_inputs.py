"""Scenes for the output-stationary convolutions of levels 2-4 (k_conv: conv_kernels.inc.h) and what they make the kernel do,
computed on the CPU: per 16-row tile of the device's row order the number of present offsets `nk` of the 3x3x3x3 map, and the
child octants present under the tile (the `omask` the fused convtr6p4s2 and k_upconv skip by).

A tile's unit list is U = nk * upk units (upk = C_in / 4), cut into S = 4 splits of per = roundup4(ceil(U / 4)) units:
    nk = 1, upk = 2 (block2.conv1): split 0 holds 2 of its 4 slots, splits 1-3 are empty;
    nk = 1 .. 5, 9: every remainder of the list against the splits, boundaries inside an offset (upk = 12: per = 4 at nk = 1);
    nk >= 27: several chunks of offsets per split.
How a scene gets its counts.  A `units` scene lives on the lattice of ONE level (0.4 / 0.8 / 1.6 m): items 8 lattice steps
apart along x, each an isolated voxel (the centre offset only) or a two-voxel cluster along one of the 13 directions (+d for
one row, -d for the other).  Every voxel is its own 4x4x4 block, so at that level the rows are the points in input order and a
tile is 16 consecutive points: 1 + 2 (whole clusters) + (half clusters) offsets.  Then 16 isolated voxels that exist at both
time indices (centre and dt), and a dense block (all 27 spatial offsets, all eight children per voxel; a second time slice
under part of it).  The `count` scenes hold n isolated voxels two level-4 cells apart: n rows at EVERY level."""
import itertools
import os
import sys

import numpy as np

from oracle import sps_oracle as O
from tests.helpers import CFG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

VS = CFG["MODEL"]["VOXEL_SIZE"]
LEVELS = (2, 3, 4)
DIRS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]       # the 13 directions up to sign
# tile counts around the tier sizes of the balanced tile order (order_ways = 64, 128 at levels 3-4; 128, 256 at level 2)
COUNT_ROWS = (993, 1024, 1039, 2017, 2048, 2063, 4065, 4096, 4111)                   # 63 64 65 127 128 129 255 256 257 tiles
# the seven tiles of a units scene: (isolated, whole clusters, leading half, trailing half) -> nk = 1 2 4 3 5 9 9.  They hold
# 13 clusters, one along each direction: every spatial offset occurs in a tile with a short unit list
UNIT_TILES = ("i" * 16, "i" * 15 + "<", ">" + "c" + "i" * 13, "c" + "i" * 14, "cc" + "i" * 12, "cccc" + "i" * 8, "cccc" + "i" * 8)
UNIT_NK = (1, 2, 4, 3, 5, 9, 9)


def rows_from(ijk, t):
    """[N, 6] float32 (b, x, y, z, t, label): one point at the centre of each level-0 voxel ijk."""
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    out = np.zeros((len(ijk), 6), np.float32)
    out[:, 1:4] = (ijk.astype(np.float64) + 0.5) * VS
    out[:, 4] = t
    out[:, 5] = (np.arange(len(ijk)) % 5) / 4.0
    return out


def units_scene(level):
    """Tiles of 1, 2, 4, 3, 5, 9 and 9 present offsets, a tile of voxels with a partner in the other time slice, a dense block."""
    sc = 1 << level
    half = sc // 2
    ijk, n_item, n_dir = [], 0, 0
    for tile in UNIT_TILES:
        for ch in tile:
            # the child octant of an isolated voxel cycles through 0..3: their tiles' omask is 0x0F
            o = n_item % 4
            iso = (8 * n_item * sc + (o & 1) * half, (o >> 1) * half, 0)
            base = (8 * n_item * sc, 4 * sc, 4 * sc)
            if ch == "i":
                ijk.append(iso)
                n_item += 1
                continue
            other = tuple(b + sc * x for b, x in zip(base, DIRS[n_dir]))               # cluster n_dir lies along DIRS[n_dir]
            if ch == "<":                          # a cluster's first voxel is this tile's last row ...
                ijk.append(base)
                pending = other
            elif ch == ">":                        # ... and its second voxel the next tile's first
                ijk.append(pending)
                n_dir += 1
            else:
                ijk += [base, other]
                n_dir += 1
            n_item += 1
    assert len(ijk) == 16 * len(UNIT_TILES) and n_dir == len(DIRS)
    both = [(8 * (n_item + i) * sc, 0, 0) for i in range(16)]                      # at t = 1 and t = 0
    # dense: 8^3 voxels of the finer level = a whole 4x4x4 block of this one, every voxel with all eight children
    g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3) * half + np.array([0, 16 * sc, 0])
    g0 = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3) * sc + np.array([0, 16 * sc, 0])
    return np.concatenate([rows_from(ijk, 1), rows_from(both, 1), rows_from(g, 1), rows_from(both, 0), rows_from(g0, 0)], 0)


def count_scene(n):
    """n rows and ceil(n / 16) tiles at EVERY level: isolated voxels on a 17 x 17 x . grid, two level-4 cells apart, at a
    random place inside their level-4 cell (the child octants differ from level to level and from row to row); the first
    quarter exists at both time indices, so the tiles hold one or two offsets and the balanced order has something to sort."""
    n0 = n // 4
    i = np.arange(n - n0)
    ijk = np.stack([i % 17, i // 17 % 17, i // 289], 1) * 32 + np.random.default_rng(n).integers(0, 16, (n - n0, 3))
    return np.concatenate([rows_from(ijk, 1), rows_from(ijk[:n0], 0)], 0)


def scenes():
    out = {f"units_l{l}": units_scene(l) for l in LEVELS}
    out["single"] = rows_from([(3, -5, 7)], 1)
    for n in COUNT_ROWS:
        out[f"count_{n}"] = count_scene(n)
    return out


def rows_of(want, got):
    """index into `got` of every row of `want` (the same coordinate set in two orders)."""
    assert want.shape == got.shape
    ow, og = np.lexsort(want.T[::-1]), np.lexsort(got.T[::-1])
    np.testing.assert_array_equal(want[ow], got[og])
    r = np.empty(len(want), np.int64)
    r[ow] = og
    return r


def coordinate_manager(batch):
    vox, _ = O.unique_first(O.quantize(batch[:, :5], VS))
    cm = O.CoordinateManager(vox)
    for ts in (2, 4, 8, 16):
        cm.ensure_stride(ts)
    return cm


def tile_facts(batch, cm=None):
    """level -> {"rows": V, "pres": [tiles, 81] bool, offset k = (dx+1) + 3(dy+1) + 9(dz+1) + 27(dt+1) of the 3x3x3x3 map is
    present in the tile, "nk": its row sums, "omask": [tiles] child octants (bit k = some row of the tile has a child at octant
    k = dx + 2 dy + 4 dz)} for levels 2-4, tiles in the device's row order."""
    import granularity_stats as G
    cm = cm or coordinate_manager(batch)
    rows, _ = G.level_rows(batch, VS, levels=5)
    out = {}
    for l in LEVELS:
        ts = 1 << l
        oc = cm.coords[ts].copy()
        oc[:, 1:4] //= ts
        dev_row = rows_of(oc, rows[l])
        nt = (len(oc) + 15) // 16
        pres = np.zeros((nt, 81), bool)
        for k, (_, o) in enumerate(cm.k3(ts)):
            pres[dev_row[o] >> 4, k] = True
        omask = np.zeros(nt, np.int64)
        for k, (_, o) in enumerate(cm.kdown(ts // 2)):
            np.bitwise_or.at(omask, dev_row[o] >> 4, 1 << k)
        out[l] = {"rows": len(oc), "pres": pres, "nk": pres.sum(1), "omask": omask}
    return out
