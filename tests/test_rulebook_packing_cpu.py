"""CPU model of the half-chunk rulebook (level 0 of the pair-exact convolutions; map_kernels.inc.h): the pairs of every
(64-row supertile, offset) are padded to a multiple of 8 -- a half-chunk --, the halves of a time-slice segment follow each
other, two per 16-slot chunk, and a segment with an odd number of halves gets one all-padding half that repeats the last
offset byte.  The model is built here, entry by entry, from the ORACLE's pair lists and must reproduce the counts of
tools/granularity_stats.py (vectorised, from coordinates) on a small scene and on the config-2 scene, where they are known:
154 511 chunks under 16-pair padding, 135 858 with half-chunks at level 0; 56 728 / 51 096 at level 1."""
import os
import sys

import numpy as np
import pytest

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests.helpers import CFG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

VS = CFG["MODEL"]["VOXEL_SIZE"]
SEG_CHUNKS = 108          # PX_SEG_CH: capacity of a segment, in chunks


def rows_of(want: np.ndarray, got: np.ndarray) -> np.ndarray:
    """index into `got` of every row of `want` (the same coordinate set in two orders)."""
    assert want.shape == got.shape
    ow, og = np.lexsort(want.T[::-1]), np.lexsort(got.T[::-1])
    np.testing.assert_array_equal(want[ow], got[og])
    r = np.empty(len(want), np.int64)
    r[ow] = og
    return r


def offset_bytes(counts27, gran):
    """Offset byte of every `gran`-pair granule of one (supertile, time slice) segment, padded to whole chunks."""
    b = []
    for j, n in enumerate(counts27):
        b += [j] * ((int(n) + gran - 1) // gran)
    if gran == 8 and len(b) % 2:
        b.append(b[-1])                                  # the all-padding half repeats the byte before it
    return b


def model(batch, level):
    """(chunks under 16-pair padding, chunks with half-chunks, two-offset chunks) per supertile, from the oracle's pairs."""
    import granularity_stats as G
    vox, _ = O.unique_first(O.quantize(batch[:, :5], VS))
    cm = O.CoordinateManager(vox)
    ts = 1 << level
    if ts > 1:
        cm.ensure_stride(ts)
    oc = cm.coords[ts].copy()
    oc[:, 1:4] //= ts                                    # units of the level's stride
    rows, _ = G.level_rows(batch, VS, levels=level + 1)
    dev_row = rows_of(oc, rows[level])                   # oracle row -> row in the library's order
    nst = (len(oc) + 63) // 64
    n = np.zeros((nst, 81), np.int64)
    for k, (_, o) in enumerate(cm.k3(ts)):
        n[:, k] = np.bincount(dev_row[o] >> 6, minlength=nst)
    c16, chh, mixed = np.zeros(nst, np.int64), np.zeros(nst, np.int64), np.zeros(nst, np.int64)
    for st in range(nst):
        for seg in range(3):
            cnt = n[st, 27 * seg:27 * seg + 27]
            b16, b8 = offset_bytes(cnt, 16), offset_bytes(cnt, 8)
            assert len(b8) % 2 == 0 and len(b8) // 2 <= len(b16) <= SEG_CHUNKS      # never more capacity than today
            assert 8 * len(b8) >= cnt.sum()
            c16[st] += len(b16)
            chh[st] += len(b8) // 2
            mixed[st] += sum(b8[2 * c] != b8[2 * c + 1] for c in range(len(b8) // 2))
    return c16, chh, mixed, G.chunk_counts(G.presence(rows[level]))


def test_half_chunk_model_small_scene():
    batch = synthetic.small_scene(seed=11, n_scan=2500)
    for level in (0, 1):
        c16, chh, mixed, tool = model(batch, level)
        for got, want in zip((c16, chh, mixed), tool):
            np.testing.assert_array_equal(got, want)
        assert (chh <= c16).all() and chh.sum() < c16.sum()


def test_half_chunk_model_config2_scene():
    batch = synthetic.make_scene(scan_seed=1)["batch"]
    known = {0: (154_511, 135_858), 1: (56_728, 51_096)}
    for level in (0, 1):
        c16, chh, mixed, tool = model(batch, level)
        for got, want in zip((c16, chh, mixed), tool):
            np.testing.assert_array_equal(got, want)
        assert (int(c16.sum()), int(chh.sum())) == known[level]
        assert (chh <= c16).all()
