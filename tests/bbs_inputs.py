"""The inputs that tests/test_bbs_cpu.py and tests/test_hip_bbs.py share: small hand-built maps and scans for the global
search that go through the wrapper (the module docstring of tests/test_hip_bbs.py lists what they cover), and the
restatement of each case, computed once.  The cases that need the raw ABI are in tests/bbs_edge_inputs.py."""
import functools
import math

import numpy as np

from tests import bbs_reference as BR
from tests import localiser_reference as LR

R = 0.5                      # cell edge
LEAF = 0.05                  # thinning: far below the spacing of the generated points
MAP_Z = (0.0, 2.0)
SCAN_Z = (-0.5, 1.5)         # of the frame T_up makes
I0, J0 = -5, 3               # the lowest cell of the hand-built map: not the origin
T_TILT = LR.perturbation(0.0, 0.0, 0.25, 0.0, pitch_deg=2.0)   # a T_up that is not the identity: height and pitch


def grid_map(seed, W=37, H=21, fill=0.22):
    """map points [M, 3] float64 whose slice MAP_Z gives a W x H grid at (I0, J0): one point in the middle of every occupied
    cell of a random, hence asymmetric, pattern (two opposite corners always occupied), and clutter above the slice that
    reaches beyond the grid on every side"""
    rng = np.random.default_rng(seed)
    occ = rng.random((H, W)) < fill
    occ[0, 0] = occ[H - 1, W - 1] = True
    j, i = np.nonzero(occ)
    pts = np.stack([R * (I0 + i + 0.5), R * (J0 + j + 0.5), np.full(len(i), 1.0)], axis=1)
    clutter = np.stack([rng.uniform(R * (I0 - 9), R * (I0 + W + 9), 40), rng.uniform(R * (J0 - 9), R * (J0 + H + 9), 40),
                        rng.uniform(2.5, 4.0, 40)], axis=1)
    return np.concatenate([pts, clutter])


def planar(x, y, yaw):
    T = np.eye(4)
    T[:2, :2] = [[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]]
    T[:2, 3] = [x, y]
    return T


def scan_of(map_xyz, pose, n_on_map, seed, T_up=None, extra=()):
    """rows float32 [n, 4] in the sensor frame: ``n_on_map`` points of the map's slice seen from ``pose`` (4x4, the pose of
    the frame that T_up makes), then the rows of ``extra`` (given in that frame too), then points below and above the scan
    slice"""
    rng = np.random.default_rng(seed)
    in_slice = map_xyz[(map_xyz[:, 2] >= MAP_Z[0]) & (map_xyz[:, 2] <= MAP_Z[1])]
    pick = in_slice[rng.integers(0, len(in_slice), n_on_map)] + np.c_[rng.uniform(-0.2, 0.2, (n_on_map, 2)) * R, np.zeros(n_on_map)]
    Ti = np.linalg.inv(pose)
    up = pick @ Ti[:3, :3].T + Ti[:3, 3]
    up[:, 2] = rng.uniform(0.0, 1.0, n_on_map)                                    # inside SCAN_Z
    up = np.concatenate([up, np.asarray(extra, dtype=np.float64).reshape(-1, 3),
                         np.c_[rng.uniform(-8, 8, (12, 2)), rng.uniform(-3.0, -1.0, 12)],
                         np.c_[rng.uniform(-8, 8, (12, 2)), rng.uniform(2.5, 4.0, 12)]])
    Ui = np.linalg.inv(np.eye(4) if T_up is None else T_up)
    sensor = up @ Ui[:3, :3].T + Ui[:3, 3]
    return np.c_[sensor, np.zeros(len(sensor))].astype(np.float32)


MAP = grid_map(7)
TRUE = dict(a=5, j=9, i=17)                                                       # of 16 yaw steps


def true_pose(A=16):
    return planar(R * (I0 + TRUE["i"]) + 0.5 * R, R * (J0 + TRUE["j"]) + 0.5 * R, 2.0 * math.pi * (TRUE["a"] * A // 16) / A)


FAR = [(60.0, 0.3, 0.5), (-60.0, 0.3, 0.5), (0.3, 60.0, 0.5), (0.3, -60.0, 0.5)]  # off the grid on all four sides
EDGE = [(R * k, R * m, 0.5) for k, m in ((1, 1), (-2, 3), (4, -1), (0, 0), (-3, -3), (6, 2), (2, -5), (-7, 1))]   # on cell edges

# name -> dict(map, rows, grid (the global_grid entries), kw (the keywords of global_search)); n: points in the scan slice
CASES = {}


def _case(name, rows, n, A, map_xyz=MAP, levels=3, map_z=MAP_Z, **kw):
    kw.setdefault("scan_z", SCAN_Z)
    CASES[name] = dict(map=map_xyz, rows=rows, n=n, A=A, grid=dict(resolution=R, map_z=map_z, levels=levels), kw=kw)


SCAN7 = scan_of(MAP, true_pose(7), 255, 20)                                      # 255 distinct voxels at LEAF: checked by the CPU test
_case("main", scan_of(MAP, true_pose(), 253, 1, T_TILT, FAR), 257, 16, T_up=T_TILT)
_case("a7_n255", SCAN7, 255, 7)
_case("a1_n256_edges", scan_of(MAP, planar(R * (I0 + 17), R * (J0 + 9), 0.0), 248, 3, None, EDGE), 256, 1)
_case("n1", scan_of(MAP, true_pose(7), 1, 4), 1, 7)
_case("n0", scan_of(MAP, true_pose(7), 0, 5), 0, 7)
_case("ties_at_the_cut", scan_of(MAP, true_pose(7), 3, 6), 3, 7, frontier=40, keep=16)
_case("uncertified", scan_of(MAP, true_pose(), 253, 1, T_TILT, FAR), 257, 16, T_up=T_TILT, frontier=60, keep=8)
_case("few_leaves", scan_of(MAP, true_pose(), 253, 1, T_TILT, FAR), 257, 16, T_up=T_TILT, keep=64, min_score=100)
_case("all_pruned", SCAN7, 255, 7, min_score=256)
_case("empty_slice", SCAN7, 0, 7, scan_z=(100.0, 200.0), T_up=T_TILT)
_case("zero_map", SCAN7, 255, 7, map_z=(50.0, 60.0))
_case("one_cell", SCAN7, 255, 7, map_xyz=np.array([[0.2, 0.2, 1.0], [0.3, 0.1, 1.5]]))
_case("level0_only", SCAN7, 255, 7, levels=0)
# three chunks of k_bbs_score through the wrapper: 2544 thinned slice points (the CPU test checks the count)
_case("three_chunks", scan_of(MAP, true_pose(3), 2600, 40), 2544, 3)
# the frontier cuts lists of 3344 and more slots, which four to six workgroups of k_bbs_count / k_bbs_write compact: one
# level below the leaves, 16 yaws, scans of 3, 5 and 9 points, so that hundreds of nodes tie at every score.  The CPU test
# says where each cut falls.  984 = the roots of the 3-point scan that score 2 or 3: the frontier is filled exactly.
for _n, _seed, _fs in ((3, 30, (900, 901, 984, 1500)), (5, 30, (900, 1500)), (9, 33, (900, 1500))):
    for _f in _fs:
        _case(f"cut_n{_n}_f{_f}", scan_of(MAP, true_pose(), _n, _seed), _n, 16, levels=1, keep=64, frontier=_f)


def thinned(rows):
    return LR.downsample(rows, len(rows), LEAF)[1]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's result of a case (computed once; treat it as read-only)"""
    c = CASES[name]
    G0, i0, j0 = BR.grid(c["map"], R, c["grid"]["map_z"])
    out = BR.search(G0, c["grid"]["levels"], R, i0, j0, thinned(c["rows"]), c["A"], **c["kw"])
    out["G0"], out["i0"], out["j0"] = G0, i0, j0
    return out


@functools.lru_cache(maxsize=None)
def exhaustive(name):
    c = CASES[name]
    G0, _, _ = BR.grid(c["map"], R, c["grid"]["map_z"])
    kw = {k: v for k, v in c["kw"].items() if k in ("scan_z", "T_up")}
    return BR.exhaustive(G0, R, thinned(c["rows"]), c["A"], **kw)
