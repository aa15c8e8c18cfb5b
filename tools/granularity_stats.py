"""Live fraction of (row group, offset) slots of the level-0 3x3x3x3 map at row-group sizes 4..64, the fill of 16-pair chunks
compacted per offset inside S-row supertiles, and the fill of the 8-pair HALF-chunk rulebook (two halves, possibly of two
offsets, per chunk; every time-slice segment rounded up to a whole chunk) at levels 0 and 1 (CPU only: numpy re-creation of
the block-contiguous row order).
Config-2 scene: 1 884 588 pairs on 108 390 rows; live fraction 0.57 / 0.48 / 0.43 / 0.40 / 0.38 at 4 / 8 / 16 / 32 / 64 rows;
chunk fill 0.76 / 0.86 / 0.92 at S = 64 / 128 / 256 (154 511 / 137 695 / 127 949 chunks against 273 k (tile, offset) slots).
Half-chunks at S = 64: level 0 135 858 chunks (fill 0.867, -12.1 %), 26 % of them with two offsets; level 1 (731 494 pairs)
56 728 -> 51 096 chunks (fill 0.806 -> 0.895, -9.9 %), 20 % with two offsets."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sps_amd import synthetic
from oracle import sps_oracle as O


def pack(a):
    return (((a[:, 0].astype(np.int64) * 32 + (a[:, 4] + 16)) * (1 << 18) + (a[:, 3] + (1 << 17))) * (1 << 18)
            + (a[:, 2] + (1 << 17))) * (1 << 18) + (a[:, 1] + (1 << 17))


def block_order(u, first):
    """Voxels u [V,5] (b, x, y, z, t; unit steps) with the rank `first` of each one's earliest source -> the rows in the
    library's order: 4x4x4 blocks per (b, t) in first-occurrence order, bit order inside a block."""
    blk = np.stack([u[:, 0], u[:, 4], u[:, 3] >> 2, u[:, 2] >> 2, u[:, 1] >> 2], 1)
    bu, binv = np.unique(blk, axis=0, return_inverse=True)
    binv = binv.ravel()
    bfirst = np.full(len(bu), 1 << 62, np.int64)
    np.minimum.at(bfirst, binv, first)
    bit = ((u[:, 3] & 3) << 4) | ((u[:, 2] & 3) << 2) | (u[:, 1] & 3)
    return u[np.lexsort((bit, bfirst[binv]))], len(bu)


def level_rows(batch, voxel_size=0.1, levels=2):
    """Rows (b, x, y, z, t in units of the level's stride) of levels 0 .. levels-1 in the library's row order."""
    co = O.quantize(batch[:, :5], voxel_size)
    u, first = np.unique(co, axis=0, return_index=True)
    rows, nblocks = [], []
    for l in range(levels):
        c, nb = block_order(u, first)
        rows.append(c), nblocks.append(nb)
        # the next level: parents (x, y, z >> 1) of this level's rows, first seen at the rank of their first child row
        p = c.copy()
        p[:, 1:4] >>= 1
        u, first = np.unique(p, axis=0, return_index=True)
    return rows, nblocks


def presence(c):
    """[V,81] bool: row u has a neighbour through offset k = (dx+1) + 3(dy+1) + 9(dz+1) + 27(dt+1)."""
    V = len(c)
    ks = np.sort(pack(c))
    pres = np.zeros((V, 81), bool)
    for k in range(81):
        n = c.copy()
        n[:, 1] += k % 3 - 1; n[:, 2] += k // 3 % 3 - 1; n[:, 3] += k // 9 % 3 - 1; n[:, 4] += k // 27 - 1
        q = pack(n)
        pos = np.minimum(np.searchsorted(ks, q), V - 1)
        pres[:, k] = ks[pos] == q
    return pres


def chunk_counts(pres, S=64):
    """Per S-row supertile: chunks under 16-pair padding, chunks of the half-chunk rulebook, and how many of those hold two
    offsets.  pres: [V,81] bool in row order."""
    V = len(pres)
    n = np.pad(pres, ((0, (-V) % S), (0, 0))).reshape(-1, S, 3, 27).sum(1)     # pairs per (supertile, time slice, offset)
    ch16 = -(-n // 16)
    h = -(-n // 8)                                                              # halves per offset
    start = np.cumsum(h, -1) - h                                               # first half of the offset inside its segment
    chh = (h.sum(-1) + 1) // 2                                                 # an odd segment gets one all-padding half
    mixed = ((h > 0) & (start % 2 == 1)).sum(-1)                               # an offset that starts in a second half
    return ch16.sum((1, 2)), chh.sum(1), mixed.sum(1)


def main():
    rows, nblocks = level_rows(synthetic.make_scene(scan_seed=1)["batch"])
    pres = presence(rows[0])
    V, P = len(pres), int(pres.sum())
    print(f"rows {V}, blocks {nblocks[0]}, pairs {P} ({P / V:.2f} per row)")
    for g in (4, 8, 16, 32, 64):
        t = np.pad(pres, ((0, (-V) % g), (0, 0))).reshape(-1, g, 81).any(1)
        print(f"row groups of {g:2d}: {t.sum(1).mean():5.1f} present offsets per group, live fraction {P / (t.sum() * g):.3f}")
    for S in (64, 128, 256):
        n = np.pad(pres, ((0, (-V) % S), (0, 0))).reshape(-1, S, 81).sum(1)
        ch = np.ceil(n / 16)
        print(f"supertiles of {S:3d} rows: {int(ch.sum())} chunks of 16 pairs, fill {P / (ch.sum() * 16):.3f}, "
              f"chunks per supertile p10 / p50 / p90 = {np.percentile(ch.sum(1), 10):.0f} / {np.percentile(ch.sum(1), 50):.0f} / {np.percentile(ch.sum(1), 90):.0f}")
    for l in range(2):
        pl = pres if l == 0 else presence(rows[l])
        Pl = int(pl.sum())
        c16, chh, mixed = (int(x.sum()) for x in chunk_counts(pl))
        print(f"level {l}: {Pl} pairs; 16-pair chunks {c16} (fill {Pl / (16 * c16):.3f}); 8-pair halves, two per chunk: {chh} chunks "
              f"(fill {Pl / (16 * chh):.3f}, {100 * (chh / c16 - 1):+.1f} %), {100 * mixed / chh:.0f} % of them with two offsets")


if __name__ == "__main__":
    main()
