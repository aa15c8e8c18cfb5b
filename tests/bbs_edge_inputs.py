"""The edge cases of the global search that tests/test_bbs_cpu.py and tests/test_hip_bbs_edges.py share.  Each goes
through the raw ABI (sps_bbs_map_build / sps_bbs_search) with float64 points, a hand-chosen capacity and device count, and
names a loop, term or limit of sps_amd/csrc/bbs_kernels.inc.h:

  chunk_*       k_bbs_score: point counts on both sides of 1, 2 and 3 chunks of BBS_CHUNK = 1024 offsets, void words on
                both sides of a chunk edge, a row stride (cap) that is no multiple of 4
  seg_*         k_bbs_threshold: 1, 2, 5 and 65 scores per thread, the cut on the first and the last score of a thread's
                segment, min_score inside that segment, a score equal to cap (the last histogram bin)
  far_*         the 16-bit packing of the offsets and the storage limit of 16384 cells per axis
  count_* / frontier_*   a device count outside [0, cap]; the frontier limits 1 and 65536

The wrapper cases that cut the frontier across several workgroups of k_bbs_count / k_bbs_write ("cut_*") and the wrapper
case of three chunks are in tests/bbs_inputs.py (CASES); cut() and place() below say where a level's cut falls in the
slot list the restatement returns.  The restatement of every case is computed once."""
import functools

import numpy as np

from tests import bbs_inputs as BI
from tests import bbs_reference as BR

R = BI.R
CHUNK, SCAN_BLOCK, THR_THREADS = 1024, 1024, 1024   # BBS_CHUNK, SCAN_BLOCK, BBS_THR_THREADS of the kernels
MAX_STORE = 16384                                   # BBS_MAX_STORE

# key -> dict(G0 uint8 [H, W], L, i0, j0)
GRIDS = {}
# name -> dict(grid, pts float64 [rows, 3], cap, n_dev, A, kw (the keywords of BR.search))
RAW = {}


def _grid(key, G0, L, i0, j0):
    GRIDS[key] = dict(G0=np.ascontiguousarray(G0, dtype=np.uint8), L=L, i0=i0, j0=j0)


def _raw(name, grid, pts, A, cap=None, n_dev=None, **kw):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    kw.setdefault("scan_z", BI.SCAN_Z)
    RAW[name] = dict(grid=grid, pts=pts, cap=len(pts) if cap is None else cap, n_dev=len(pts) if n_dev is None else n_dev,
                     A=A, kw=kw)


def counted(case):
    """the points of a raw case that the search reads: the first min(cap, max(n_dev, 0)) rows"""
    return case["pts"][:min(case["cap"], max(case["n_dev"], 0))]


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = RAW[name]
    g = GRIDS[c["grid"]]
    with np.errstate(invalid="ignore", over="ignore"):
        return BR.search(g["G0"], g["L"], R, g["i0"], g["j0"], counted(c), c["A"], **c["kw"])


def reference(name):
    """the restatement's result of a raw case (computed once; treat it as read-only).  Cases that differ only in cap, with
    the same rows counted, share it: ``like`` names the first of them"""
    return _reference(RAW[name].get("like", name))


@functools.lru_cache(maxsize=None)
def _exhaustive(name):
    c = RAW[name]
    kw = {k: v for k, v in c["kw"].items() if k in ("scan_z", "T_up")}
    with np.errstate(invalid="ignore", over="ignore"):
        return BR.exhaustive(GRIDS[c["grid"]]["G0"], R, counted(c), c["A"], **kw)


def exhaustive(name):
    return _exhaustive(RAW[name].get("like", name))


# ---- where a cut falls -----------------------------------------------------------------------------------------------------
def cut(slot_scores, frontier, min_score=1):
    """the cut of one level from the scores of its slots (-1: void), as DESIGN.md 8m states it: None where the S nodes with
    score >= min_score fit the frontier; otherwise dict(t: the largest score with at least F nodes at or above it, above:
    the nodes above t, quota: F - above, ties: the slots with score t in slot order, hi: the highest score below t that a
    node has, -1 for none)"""
    sc = np.asarray(slot_scores)
    if int((sc >= max(min_score, 0)).sum()) <= frontier:
        return None
    t = int(np.sort(sc)[::-1][frontier - 1])
    above = int((sc > t).sum())
    below = sc[(sc < t) & (sc >= 0)]
    return dict(t=t, above=above, quota=frontier - above, ties=np.nonzero(sc == t)[0], hi=int(below.max()) if len(below) else -1)


def place(slot_scores, frontier, min_score=1):
    """facts about the cut of a level in terms of the 1024-slot blocks of k_bbs_count / k_bbs_write; None where nothing is
    cut.  quota_slot: the slot of the last tie kept"""
    c = cut(slot_scores, frontier, min_score)
    if c is None:
        return None
    ties, q = c["ties"], c["quota"]
    kept, dropped = ties[:q], ties[q:]
    quota_slot = int(kept[-1])
    qb = quota_slot // SCAN_BLOCK
    return dict(c, quota_slot=quota_slot, quota_block=qb, last_block=(len(slot_scores) - 1) // SCAN_BLOCK,
                kept_blocks=sorted(set((kept // SCAN_BLOCK).tolist())),
                dropped_in_quota_block=int((dropped // SCAN_BLOCK == qb).sum()),
                dropped_in_later_blocks=int((dropped // SCAN_BLOCK > qb).sum()),
                voids_before_quota=int((np.asarray(slot_scores)[:quota_slot] < 0).sum()))


# ---- a. chunk edges of k_bbs_score -----------------------------------------------------------------------------------------
_G0, _I0, _J0 = BR.grid(BI.MAP, R, BI.MAP_Z)
_grid("map_l3", _G0, 3, _I0, _J0)
# rows that give a void word and do not count for the slice: not finite, above and below the slice
SKIPPED = np.array([[np.nan, 0.0, 0.5], [0.3, 0.2, 5.0], [np.inf, 1.0, 0.5], [0.1, -0.4, -3.0]])


def slice_points(n, seed, yaw_steps=3):
    """n float64 points inside SCAN_Z: points of the map's slice as seen from BI.true_pose(yaw_steps), jittered inside their
    cells"""
    rng = np.random.default_rng(seed)
    in_slice = BI.MAP[(BI.MAP[:, 2] >= BI.MAP_Z[0]) & (BI.MAP[:, 2] <= BI.MAP_Z[1])]
    pick = in_slice[rng.integers(0, len(in_slice), n)] + np.c_[rng.uniform(-0.2, 0.2, (n, 2)) * R, np.zeros(n)]
    Ti = np.linalg.inv(BI.true_pose(yaw_steps))
    up = pick @ Ti[:3, :3].T + Ti[:3, 3]
    up[:, 2] = rng.uniform(0.0, 1.0, n)
    return up


def with_voids(pts):
    """the points with skipped rows in front, on both sides of every chunk edge they reach, and behind: the slice count
    stays len(pts)"""
    out = np.concatenate([SKIPPED[:2], pts])
    for edge in range(CHUNK, len(out) + 1, CHUNK):
        out = np.concatenate([out[:edge - 2], SKIPPED, out[edge - 2:]])
    return np.concatenate([out, SKIPPED[1:]])


CHUNK_N = (1023, 1024, 1025, 2047, 2049, 3073)
for _n in CHUNK_N:
    _p = slice_points(_n, 100 + _n)
    _raw(f"chunk_n{_n}", "map_l3", _p, 3, cap=4096)                          # the count itself on the edge
    _raw(f"chunk_n{_n}_voids", "map_l3", with_voids(_p), 3, cap=4096)        # voids on both sides of the edges
_raw("chunk_cap_is_n_1025", "map_l3", slice_points(1025, 77), 3, cap=1025)   # rows of 1025 words: no row but the first is aligned

# ---- c. the segments of k_bbs_threshold -------------------------------------------------------------------------------------
SEG_CAPS = (3, 1023, 1024, 4096, 65536)                                     # 1, 1, 2, 5 and 65 scores per thread
SEG_MIN_SCORES = (0, 1, 2)


def seg_points():
    """the three slice points of the wrapper case cut_n3_f900"""
    p = BI.thinned(BI.CASES["cut_n3_f900"]["rows"])
    return p[(p[:, 2] >= BI.SCAN_Z[0]) & (p[:, 2] <= BI.SCAN_Z[1])]


SEG_FRONTIERS = (200, 400, 1000)       # on three levels the 3-point scan is cut at 3, 2 and 1 (the CPU test checks it)
for _cap in SEG_CAPS:
    for _f in SEG_FRONTIERS:
        for _ms in SEG_MIN_SCORES:
            _raw(f"seg_cap{_cap}_f{_f}_ms{_ms}", "map_l3", seg_points(), 16, cap=_cap, n_dev=3, keep=64, frontier=_f, min_score=_ms)
            RAW[f"seg_cap{_cap}_f{_f}_ms{_ms}"]["like"] = f"seg_cap{SEG_CAPS[0]}_f{_f}_ms{_ms}"

# the last histogram bin: every point of the scan in one 3 x 3 block of cells of an all-ones grid, so the best nodes score cap
_grid("ones_9x9", np.ones((9, 9), np.uint8), 2, -4, -4)
_rng = np.random.default_rng(5)
_p = np.c_[_rng.uniform(0.0, 3.0 * R, (1024, 2)), _rng.uniform(0.0, 1.0, 1024)]
_raw("seg_last_bin", "ones_9x9", _p, 1, cap=1024, keep=8, frontier=64)         # 49 leaves score cap: all above the cut
_raw("seg_last_bin_f32", "ones_9x9", _p, 1, cap=1024, keep=8, frontier=32)     # the cut itself in the last bin, ties dropped

# ---- d. the storage limit and the 16-bit packing ----------------------------------------------------------------------------
# (cell offset along the long axis at yaw 0, the places inside the cell): one point each.  +-16383 are legal words that no
# node brings onto the storage, +-16384 are void; three points make the far hits outweigh anything the near ones find
FAR_POINTS = ((0, (0.5,)), (16376, (0.25, 0.5, 0.75)), (-16376, (0.5,)), (16375, (0.25, 0.5, 0.75)), (-16375, (0.5,)),
              (16383, (0.5,)), (-16383, (0.5,)), (16384, (0.5,)), (-16384, (0.5,)),
              (1, (0.5,)), (3, (0.5,)), (4, (0.5,)), (-2, (0.5,)), (-5, (0.5,)))


def far_line(seed=0, n=16377, fill=0.3):
    """occupancy along the long axis: cells 0 and n - 1, a pattern beside each, a gap, and a random rest"""
    rng = np.random.default_rng(seed)
    occ = (rng.random(n) < fill).astype(np.uint8)
    occ[:8] = 0
    occ[-8:] = 0
    occ[[0, 1, 3, 4, n - 1, n - 3, n - 6]] = 1
    return occ


def far_points(axis, without=()):
    """the points of FAR_POINTS along ``axis`` (0: x, 1: y), without those of the offsets in ``without``, at exactly 0 along
    the other axis: at yaw 0 the other offset is 0, at pi it is 0 or -1 by the sign of the product with sin(pi) = 1.2e-16"""
    d = np.array([c + f for c, fs in FAR_POINTS if c not in without for f in fs], dtype=np.float64)
    p = np.zeros((len(d), 3))
    p[:, axis] = R * d
    p[:, 2] = 0.5
    return p


_occ = far_line()
_grid("far_w_l3", _occ[None, :], 3, -8000, 11)                               # 16377 x 1: Ws = 16384
_grid("far_h_l3", _occ[:, None], 3, 9, -8100)                                # 1 x 16377: Hs = 16384
_grid("far_w_l0", np.concatenate([_occ, [0, 1, 0, 0, 1, 1, 0]])[None, :], 0, -8000, 11)   # 16384 x 1 with no pad
for _A in (2, 4):
    _raw(f"far_w_l3_a{_A}", "far_w_l3", far_points(0), _A, cap=64, frontier=4096)
    _raw(f"far_h_l3_a{_A}", "far_h_l3", far_points(1), _A, cap=64, frontier=4096)
_raw("far_w_l0_a2", "far_w_l0", far_points(0), 2, cap=64, frontier=8192)

# level 7 of a 130 x 130 grid: the root (0, 0) reads pooled cells at x, y = -127 .. -1 through the negative pad
_rng = np.random.default_rng(11)
_grid("pad_l7", (_rng.random((130, 130)) < 0.05).astype(np.uint8), 7, 40, -70)
_raw("pad_l7", "pad_l7", np.c_[_rng.uniform(-64.0, 64.0, (200, 2)), _rng.uniform(0.0, 1.0, 200)], 3, cap=256, frontier=4096)

# ---- e. the device count and the frontier limits ----------------------------------------------------------------------------
_p = slice_points(300, 9)
_raw("count_at_cap", "map_l3", _p, 3, cap=256, n_dev=256)
_raw("count_beyond_cap", "map_l3", _p, 3, cap=256, n_dev=1256)
_raw("count_zero", "map_l3", _p, 3, cap=256, n_dev=0)
_raw("count_negative", "map_l3", _p, 3, cap=256, n_dev=-5)
_grid("one_cell", np.ones((1, 1), np.uint8), 3, 0, 0)
_raw("frontier_1", "one_cell", BI.thinned(BI.SCAN7), 4, cap=512, frontier=1)
_raw("frontier_1_min_score_0", "one_cell", BI.thinned(BI.SCAN7), 4, cap=512, frontier=1, min_score=0)   # its one leaf is kept
_raw("frontier_65536", "map_l3", _p, 16, cap=512, frontier=65536)
