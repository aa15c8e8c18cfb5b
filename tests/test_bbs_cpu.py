"""CPU tests of the numpy restatement of the global search (tests/bbs_reference.py), of the inputs the GPU test re-uses
(tests/bbs_inputs.py), and of the argument checks and driver options that need no device.  No GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from sps_amd import synthetic
from tests import bbs_inputs as BI
from tests import bbs_reference as BR
from tests import localiser_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(n_azimuth=400, n_beams=32)
# the synthetic corridor: cells of 1 m and 10 degree steps keep the exhaustive scorer quick; the slice leaves the ground
# (z = -1.8) out and keeps walls and poles
CORRIDOR = dict(grid=dict(resolution=1.0, map_z=(-1.0, 3.0), levels=3), scan_z=(-1.0, 3.0), yaw_steps=36,
                truth=(2.3, 0.4, 40.0), x_offset=2.0, seed=1)


def corridor_scene():
    x, y, yaw = CORRIDOR["truth"]
    T = BI.planar(x, y, math.radians(yaw))
    world = synthetic.lidar_scan(CORRIDOR["seed"], x_offset=CORRIDOR["x_offset"], **KW)
    Ti = np.linalg.inv(T)
    scan = np.c_[world[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3], world[:, 3]].astype(np.float32)
    return dict(map_xyz=synthetic.build_map(**KW)[:, :3].astype(np.float64), scan=scan, T_true=T)


def leaf_of(k, W, H):
    return k // W // H, k // W % H, k % W


# ---- 1. the grid and the bound -------------------------------------------------------------------------------------------
def test_pooled_levels_follow_the_definition_and_the_recurrence():
    rng = np.random.default_rng(0)
    G0 = (rng.random((11, 13)) < 0.2).astype(np.uint8)
    for l in range(4):
        Gl, p = BR.pooled(G0, l), (1 << l) - 1
        assert Gl.shape == (11 + p, 13 + p)
        for _ in range(200):
            x, y = int(rng.integers(-p - 2, 15)), int(rng.integers(-p - 2, 13))
            want = 0
            for dj in range(1 << l):
                for di in range(1 << l):
                    if 0 <= y + dj < 11 and 0 <= x + di < 13:
                        want = max(want, int(G0[y + dj, x + di]))
            assert int(BR.lookup(Gl, l, np.array([x]), np.array([y]))[0]) == want
    L = 3
    for l in range(1, L + 1):                                               # what the device computes: level l from level l - 1
        below, h = BR.stored(G0, L, l - 1), 1 << (l - 1)
        big = np.zeros((below.shape[0] + h, below.shape[1] + h), np.uint8)
        big[:below.shape[0], :below.shape[1]] = below
        rec = np.maximum(np.maximum(big[:-h, :-h], big[:-h, h:]), np.maximum(big[h:, :-h], big[h:, h:]))
        assert np.array_equal(rec, BR.stored(G0, L, l))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_nodes_score_bounds_every_leaf_below_it(seed):
    rng = np.random.default_rng(seed)
    H, W, A, L = 13, 19, 5, 3
    G0 = (rng.random((H, W)) < 0.3).astype(np.uint8)
    pts = np.c_[rng.uniform(-4, 4, (40, 2)), np.zeros(40)]
    offs, n = BR.offsets(pts, np.eye(4), (-1, 1), 0.5, BR.yaw_table(A))
    assert n == 40
    leaves = BR.exhaustive(G0, 0.5, pts, A, scan_z=(-1, 1))
    for l in range(1, L + 1):
        step = 1 << l
        nodes = np.array([(a, j, i) for a in range(A) for j in range(0, H, step) for i in range(0, W, step)], np.int64)
        sc = BR.score_nodes(BR.pooled(G0, l), l, nodes, offs)
        for (a, j, i), s in zip(nodes.tolist(), sc.tolist()):
            assert s >= leaves[a, j:j + step, i:i + step].max()
    nodes0 = np.array([(a, j, i) for a in range(A) for j in range(H) for i in range(W)], np.int64)
    assert np.array_equal(BR.score_nodes(BR.pooled(G0, 0), 0, nodes0, offs).reshape(A, H, W), leaves)


# ---- 2. the cases of the GPU test ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BI.CASES))
def test_the_certified_prefix_is_the_exhaustive_rankings(name):
    c, ref = BI.CASES[name], BI.reference(name)
    assert ref["n_slice"] == c["n"]                                          # the thinning kept every generated point
    K = len(ref["index"])
    ids, sc = BR.exhaustive_ranking(BI.exhaustive(name), K, c["kw"].get("min_score", 1))
    n = ref["certified"]
    assert ref["index"][:n].tolist() == ids[:n].tolist() and ref["score"][:n].tolist() == sc[:n].tolist()
    assert ref["n_found"] <= len(ids) or ref["n_found"] == K
    if c["kw"].get("frontier", 16384) == 16384:                              # a generous frontier cuts nothing
        assert ref["certified"] == ref["n_found"] == min(K, len(ids)) and ref["kept"].max() <= 16384
        assert ref["index"][:n].tolist() == ids.tolist()
    assert (ref["index"][ref["n_found"]:] == -1).all()
    first = ref["poses"][0] if ref["n_found"] else np.asarray(c["kw"].get("T_up", np.eye(4)))
    assert all(p.tobytes() == first.tobytes() for p in ref["poses"][ref["n_found"]:])


def test_the_cases_take_the_paths_they_are_named_for():
    ref = {n: BI.reference(n) for n in BI.CASES}
    H, W = ref["main"]["G0"].shape
    assert (W, H) == (37, 21) and (BI.reference("main")["i0"], BI.reference("main")["j0"]) == (BI.I0, BI.J0)
    assert ref["one_cell"]["G0"].shape == (1, 1) and ref["one_cell"]["G0"][0, 0] == 1 and ref["one_cell"]["n_found"] >= 1
    assert ref["zero_map"]["G0"].shape == (1, 1) and ref["zero_map"]["G0"][0, 0] == 0 and ref["zero_map"]["n_found"] == 0
    assert ref["main"]["certified"] == 8 and ref["few_leaves"]["candidates"][0] < 16 * H * W // 3    # the bound pruned most
    assert ref["main"]["candidates"][1] < 4 * ref["main"]["kept"][2]                         # children fell outside the grid
    # the best leaf of the asymmetric hand-built scene is the true one, to a cell and a yaw step
    a, j, i = leaf_of(int(ref["main"]["index"][0]), W, H)
    assert abs(a - BI.TRUE["a"]) <= 1 and abs(j - BI.TRUE["j"]) <= 1 and abs(i - BI.TRUE["i"]) <= 1
    assert ref["main"]["score"][0] > ref["main"]["score"][1]
    # the frontier cuts the first level between nodes of equal score: position decides
    c = BI.CASES["ties_at_the_cut"]
    t = ref["ties_at_the_cut"]
    nodes = np.array([(a, j, i) for a in range(7) for j in range(0, H, 8) for i in range(0, W, 8)], np.int64)
    offs, _ = BR.offsets(BI.thinned(c["rows"]), np.eye(4), BI.SCAN_Z, BI.R, BR.yaw_table(7))
    sc = np.sort(BR.score_nodes(BR.pooled(t["G0"], 3), 3, nodes, offs))[::-1]
    assert sc[39] == sc[40] >= 1 and t["kept"][3] == 40 and t["dropped_bound"] >= sc[40]
    assert 0 < t["certified"] < t["n_found"] == 16
    assert ref["uncertified"]["certified"] < 8 == ref["uncertified"]["n_found"]
    assert 0 < ref["few_leaves"]["n_found"] < 64 and ref["few_leaves"]["certified"] == ref["few_leaves"]["n_found"]
    assert ref["all_pruned"]["n_found"] == 0 and ref["all_pruned"]["dropped_bound"] == 255 and ref["all_pruned"]["kept"].sum() == 0
    assert ref["empty_slice"]["n_slice"] == 0 and ref["empty_slice"]["n_found"] == 0
    assert ref["empty_slice"]["poses"][0].tobytes() == BI.T_TILT.tobytes()
    assert ref["n0"]["n_found"] == 0 and ref["n1"]["score"].tolist() == [1] * 8
    assert ref["level0_only"]["index"].tolist() == ref["a7_n255"]["index"].tolist()
    # points on cell edges: with one yaw (cos = 1, sin = 0 exactly) the quotient is an integer and the floor keeps it
    e = BR.offsets(np.array(BI.EDGE), np.eye(4), BI.SCAN_Z, BI.R, BR.yaw_table(1))[0][0]
    assert e[0].tolist() == [1, -2, 4, 0, -3, 6, 2, -7] and e[1].tolist() == [1, 3, -1, 0, -3, 2, -5, 1]


def test_leaf_poses_are_planar_motions_of_t_up():
    ref = BI.reference("main")
    H, W = ref["G0"].shape
    a, j, i = leaf_of(int(ref["index"][0]), W, H)
    want = BI.planar(BI.R * (ref["i0"] + i), BI.R * (ref["j0"] + j), 2.0 * math.pi * a / 16) @ BI.T_TILT
    assert np.abs(ref["poses"][0] - want).max() < 1e-12
    assert ref["poses"][0][2:].tobytes() == BI.T_TILT[2:].tobytes()


# ---- 3. a scene: where is the scan? ----------------------------------------------------------------------------------------
def test_the_exhaustive_best_leaf_of_the_synthetic_corridor_is_the_true_pose():
    s = corridor_scene()
    g = CORRIDOR["grid"]
    G0, i0, j0 = BR.grid(s["map_xyz"], g["resolution"], g["map_z"])
    pts = LR.downsample(s["scan"], len(s["scan"]), 0.2)[1]
    ex = BR.exhaustive(G0, g["resolution"], pts, CORRIDOR["yaw_steps"], scan_z=CORRIDOR["scan_z"])
    ids, sc = BR.exhaustive_ranking(ex, 2)
    H, W = G0.shape
    a, j, i = leaf_of(int(ids[0]), W, H)
    x, y, yaw = CORRIDOR["truth"]
    r = g["resolution"]
    assert abs(a - yaw / (360.0 / CORRIDOR["yaw_steps"])) <= 1
    assert abs(r * (i0 + i) - x) <= r and abs(r * (j0 + j) - y) <= r       # the leaf's corner, within one cell of the truth
    assert sc[0] > sc[1]
    # the search finds the same leaves, and with min_score at the fourth best score it scores a fraction of the nodes
    ids4, sc4 = BR.exhaustive_ranking(ex, 4)
    high = BR.search(G0, g["levels"], r, i0, j0, pts, CORRIDOR["yaw_steps"], keep=4, min_score=int(sc4[-1]), scan_z=CORRIDOR["scan_z"])
    assert high["certified"] == 4 and high["index"].tolist() == ids4.tolist() and high["score"].tolist() == sc4.tolist()
    assert high["candidates"].sum() < CORRIDOR["yaw_steps"] * H * W // 4


# ---- 4. argument checks and the driver --------------------------------------------------------------------------------------
def test_global_arguments_are_checked_before_any_device_work():
    from sps_amd.localiser import NDTLocaliser
    m = np.array([[0.1, 0.1, 0.5], [3.0, 2.0, 0.5]])
    for grid, match in ((dict(resolution=0.0), "resolution"), (dict(levels=8), "levels"), (dict(levels=-1), "levels"),
                        (dict(cells=3), "unknown"), (dict(map_z=(float("nan"), 1.0)), "map_z")):
        with pytest.raises(ValueError, match=match):
            NDTLocaliser(m, global_grid=grid, device="no-such-device")
    with pytest.raises(ValueError, match="capacity"):
        NDTLocaliser(m, global_grid=dict(), capacity=1 << 17, device="no-such-device")
    with pytest.raises(ValueError, match="source='points'"):
        NDTLocaliser(m, global_grid=dict(), source="cells", device="no-such-device")
    with pytest.raises(ValueError, match="cells per axis"):
        NDTLocaliser(np.array([[0.0, 0.0, 0.5], [9000.0, 0.0, 0.5]]), global_grid=dict(resolution=0.5), device="no-such-device")
    rows = np.zeros((1, 4), np.float32)
    loc = object.__new__(NDTLocaliser)                                   # the refusals look at nothing but these
    loc.source = "cells"
    for call in (lambda: loc.global_search(rows, 1, 8), lambda: loc.localise_global(rows, 1, 8)):
        with pytest.raises(ValueError, match="source='points'"):
            call()
    loc.source = "points"
    for call in (lambda: loc.global_search(rows, 1, 8), lambda: loc.localise_global(rows, 1, 8), lambda: loc.global_level(0)):
        with pytest.raises(ValueError, match="global_grid"):
            call()
    loc._global = NDTLocaliser._checked_global_grid(dict(resolution=0.5, levels=1), np.array([[0.0, 0.0, 0.5], [49.9, 29.9, 0.5]]), 1024)
    assert (loc._global["W"], loc._global["H"]) == (100, 60)
    for fn in (loc.global_search, loc.localise_global):
        for kw in (dict(keep=0), dict(keep=65)):
            with pytest.raises(ValueError, match="keep"):
                fn(rows, 1, 8, **kw)
        with pytest.raises(ValueError, match="exceed 4 \\* frontier"):
            fn(rows, 1, 72, frontier=1000)                               # 72 * 30 * 50 root nodes
        for kw in (dict(frontier=0), dict(frontier=65537), dict(min_score=-1)):
            with pytest.raises(ValueError, match="frontier"):
                fn(rows, 1, 8, **kw)
        with pytest.raises(ValueError, match="yaw_steps"):
            fn(rows, 1, 0)
        with pytest.raises(ValueError, match="T_up"):
            fn(rows, 1, 8, T_up=np.full((4, 4), np.nan))
        with pytest.raises(ValueError, match="scan_z"):
            fn(rows, 1, 8, scan_z=(0.0, float("nan")))
    big = NDTLocaliser._checked_global_grid(dict(resolution=0.5, levels=7), np.array([[0.0, 0.0, 0.5], [999.9, 599.9, 0.5]]), 1024)
    loc._global = big                                                    # 2000 x 1200 cells: 4096 yaws overflow the id
    with pytest.raises(ValueError, match="int32"):
        loc.global_search(rows, 1, 4096, frontier=65536)
    assert loc.global_search.__doc__ and loc.localise_global_filtered.__doc__


def test_the_host_grid_is_the_restatements():
    from sps_amd.localiser import NDTLocaliser
    for name in ("main", "zero_map", "one_cell"):
        c = BI.CASES[name]
        g = NDTLocaliser._checked_global_grid(c["grid"], np.ascontiguousarray(c["map"], dtype=np.float64), 1024)
        G0, i0, j0 = BR.grid(c["map"], BI.R, c["grid"]["map_z"])
        assert np.array_equal(g["G0"], G0) and (g["i0"], g["j0"]) == (i0, j0)
    assert NDTLocaliser._checked_global_grid(None, None, 1 << 20) is None


def test_the_binding_knows_the_global_search_entry_points():
    from sps_amd import _native
    for name in ("sps_bbs_map_build", "sps_bbs_map_level", "sps_bbs_search_scratch", "sps_bbs_search"):
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
    assert _native.lib.sps_version() == _native.ABI_VERSION == 202        # additive: the ABI version does not change
    s = _native.lib.sps_bbs_search_scratch
    assert s(65536, 72, 16384) > 72 * 65536 * 4 and s(1000, 8, 64) < s(1000, 8, 128) and s(1000, 8, 64) < s(1000, 9, 64)
    assert s(0, 1, 1) > 0
    for bad in ((65537, 8, 64), (-1, 8, 64), (100, 0, 64), (100, 4097, 64), (100, 8, 0), (100, 8, 65537)):
        assert s(*bad) == -1


def test_the_drivers_list_the_global_options():
    script = os.path.join(ROOT, "scripts", "filter_sequence.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-1500:]
    for flag in ("--global-start", "--global-resolution", "--global-map-z", "--global-scan-z", "--global-yaw-steps",
                 "--global-levels", "--global-frontier"):
        assert flag in r.stdout
    r = subprocess.run([sys.executable, script, "--synthetic", "2", "--global-start"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--global-start needs --localise --localiser ndt" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "localiser_timing.py"), "--help"], capture_output=True,
                       text=True, cwd=ROOT)
    assert r.returncode == 0 and "--global" in r.stdout
