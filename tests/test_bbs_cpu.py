"""CPU tests of the numpy restatement of the global search (tests/bbs_reference.py), of the inputs the GPU tests re-use
(tests/bbs_inputs.py, tests/bbs_edge_inputs.py) -- among them that every edge case sits where it claims, asserted from
the restatement's output alone -- and of the argument checks and driver options that need no device.  No GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from sps_amd import synthetic
from tests import bbs_edge_inputs as BE
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


# ---- 5. the edge cases: each sits where it claims ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BE.RAW))
def test_the_certified_prefix_of_an_edge_case_is_the_exhaustive_rankings(name):
    c, ref = BE.RAW[name], BE.reference(name)
    K = len(ref["index"])
    ids, sc = BR.exhaustive_ranking(BE.exhaustive(name), K, c["kw"].get("min_score", 1))
    n = ref["certified"]
    assert ref["index"][:n].tolist() == ids[:n].tolist() and ref["score"][:n].tolist() == sc[:n].tolist()
    assert ref["n_found"] <= len(ids) or ref["n_found"] == K
    assert (ref["index"][ref["n_found"]:] == -1).all()
    for l, (slots, scores) in enumerate(zip(ref["slot_lists"], ref["slot_scores"])):    # the slot lists are the candidates
        assert slots[slots >= 0].tolist() == ref["candidate_lists"][l].tolist() and ((slots < 0) == (scores < 0)).all()
        assert len(slots) == (4 * ref["kept"][l + 1] if l < len(ref["kept"]) - 1 else ref["candidates"][l])


def in_slice(pts):
    with np.errstate(invalid="ignore"):
        return (pts[:, 2] >= BI.SCAN_Z[0]) & (pts[:, 2] <= BI.SCAN_Z[1]) & np.isfinite(pts).all(axis=1)


def test_the_chunk_cases_put_the_point_count_and_the_voids_on_the_chunk_edges():
    """k_bbs_score: for (c0 = 0; c0 < n; c0 += BBS_CHUNK), q1 = ceil((n - c0) / 4), the fills p + k < n"""
    assert BE.CHUNK_N == (1023, 1024, 1025, 2047, 2049, 3073)
    for n in BE.CHUNK_N:
        clean, voids = BE.RAW[f"chunk_n{n}"], BE.RAW[f"chunk_n{n}_voids"]
        assert clean["cap"] == voids["cap"] == 4096 and clean["n_dev"] == len(clean["pts"]) == n and in_slice(clean["pts"]).all()
        a, b = BE.reference(f"chunk_n{n}"), BE.reference(f"chunk_n{n}_voids")
        assert a["n_slice"] == b["n_slice"] == n                              # exactly n slice points, with and without voids
        m = in_slice(BE.counted(voids))
        assert voids["n_dev"] == len(m) > n and int(m.sum()) == n
        assert not m[:2].any() and not m[-3:].any()                           # void words in front and behind
        edges = list(range(BE.CHUNK, len(m), BE.CHUNK))
        assert len(edges) == (n + 2) // BE.CHUNK >= 1                         # and on both sides of every chunk edge
        for e in edges:
            assert not m[e - 2:e + 2].any() and m[e - 3] and m[e + 2]
        assert a["index"].tolist() == b["index"].tolist() and a["score"].tolist() == b["score"].tolist()   # voids score nothing
        assert a["candidates"].tolist() == b["candidates"].tolist() and a["certified"] == 8
    c = BE.RAW["chunk_cap_is_n_1025"]
    assert c["cap"] == c["n_dev"] == len(c["pts"]) == BE.reference("chunk_cap_is_n_1025")["n_slice"] == 1025
    w = BI.CASES["three_chunks"]                                              # the wrapper: the third chunk is partial
    pts = BI.thinned(w["rows"])
    assert len(pts) <= 4096 and 2048 < BI.reference("three_chunks")["n_slice"] == w["n"] < 3072


CUT_CASES = sorted(n for n in BI.CASES if n.startswith("cut_"))


def cut_places():
    """(name, level, place) of every level of the cut cases that the frontier cuts"""
    out = []
    for name in CUT_CASES:
        ref, F = BI.reference(name), BI.CASES[name]["kw"]["frontier"]
        for l in (1, 0):
            p = BE.place(ref["slot_scores"][l], F)
            if p is not None:
                out.append((name, l, p))
    return out


def test_the_cut_cases_cut_across_the_workgroups_of_the_compaction():
    """k_bbs_count / k_bbs_write: k = ra + min(rt, quota) with base_a, base_t > 0, *slots_out by a last workgroup that is
    not workgroup 0; k_bbs_top: 64 results out of more than 1024 tied leaves"""
    assert len(CUT_CASES) == 8
    for name in CUT_CASES:
        ref, c = BI.reference(name), BI.CASES[name]
        F = c["kw"]["frontier"]
        assert c["grid"]["levels"] == 1 and c["A"] == 16 and ref["candidates"][1] == 3344 > 3 * BE.SCAN_BLOCK
        assert ref["kept"].tolist() == [F, F] and ref["n_found"] == 64          # both levels cut
        for l in (1, 0):                                                       # the cut of cut() is the restatement's
            sc, slots = ref["slot_scores"][l], ref["slot_lists"][l]
            p = BE.place(sc, F)
            keep = (sc > p["t"])
            keep[p["ties"][:p["quota"]]] = True
            assert slots[keep].tolist() == ref["kept_lists"][l].tolist() and 1 <= p["quota"] <= len(p["ties"])
            assert len(set((np.nonzero(keep)[0] // BE.SCAN_BLOCK).tolist())) >= 3   # the kept are spread over the blocks
        assert len(ref["slot_scores"][0]) > 3 * BE.SCAN_BLOCK and len(set(ref["score"].tolist())) <= 4   # 64 results, few scores
    places = cut_places()
    # the slot that uses up the quota is past the first block and not in the last
    assert any(p["quota_slot"] >= BE.SCAN_BLOCK and p["quota_block"] < p["last_block"] for _, _, p in places)
    assert any(len(p["kept_blocks"]) >= 2 for _, _, p in places)                # ties kept in two blocks and more
    assert any(p["dropped_in_quota_block"] > 0 and p["dropped_in_later_blocks"] > 0 for _, _, p in places)
    # all of it at once, with voids in front of the quota slot: slot index and candidate rank differ
    full = [(n, l) for n, l, p in places if p["quota_slot"] >= BE.SCAN_BLOCK and p["quota_block"] < p["last_block"] and
            len(p["kept_blocks"]) >= 2 and p["dropped_in_quota_block"] > 0 and p["dropped_in_later_blocks"] > 0 and
            p["voids_before_quota"] > 0]
    assert ("cut_n3_f1500", 0) in full and ("cut_n5_f900", 0) in full
    assert any(l == 1 and n == "cut_n3_f900" for n, l, p in places if p["quota_block"] == 2 and p["last_block"] == 3)
    # up to six blocks at level 0
    assert max(p["last_block"] for _, l, p in places if l == 0) == 5
    # the frontier filled exactly.  In the kernel's terms (the cut score t is the largest with F nodes at or above it) the
    # quota is at least 1 by construction and here equals the number of ties: no tie is dropped and the bound comes from
    # `hi`.  Read from below -- with `hi` as the score where the cut falls -- the same level has a quota of 0: the frontier is
    # full of scores above `hi` and every node at `hi` is dropped.
    ref = BI.reference("cut_n3_f984")
    p = BE.place(ref["slot_scores"][1], 984)
    sc = ref["slot_scores"][1]
    assert p["t"] == 2 and p["quota"] == len(p["ties"]) == 697 and p["hi"] == 1
    assert int((sc > p["hi"]).sum()) == 984 and int((sc == p["hi"]).sum()) > 0 and len(p["kept_blocks"]) == 4
    # the 9-point scan at F = 900: the certificate depends on a cut that crosses blocks
    assert BI.reference("cut_n9_f900")["certified"] == 28
    assert 0 < BI.reference("cut_n3_f900")["certified"] < 64 == BI.reference("cut_n3_f1500")["certified"]
    # k_bbs_top: more than 1024 leaves, 64 results that tie at two or three scores: the id decides across the waves
    for n in ("cut_n3_f1500", "cut_n5_f1500", "cut_n9_f1500"):
        ref = BI.reference(n)
        assert ref["kept"][0] == 1500 > 1024 and np.bincount(ref["score"]).max() >= 8


def test_the_segment_cases_reach_every_cut_score_and_the_last_bin():
    """k_bbs_threshold: seg = (cap + 1024) / 1024 scores per thread; the cut on the first and the last score of a segment"""
    assert [(cap + BE.THR_THREADS) // BE.THR_THREADS for cap in BE.SEG_CAPS] == [1, 1, 2, 5, 65]
    assert len(BE.seg_points()) == 3
    cuts = {}
    for F in BE.SEG_FRONTIERS:
        for ms in BE.SEG_MIN_SCORES:
            ref = BE.reference(f"seg_cap3_f{F}_ms{ms}")
            assert ref["n_slice"] == 3 and max(int(s.max()) for s in ref["slot_scores"]) == 3
            for l, sc in enumerate(ref["slot_scores"]):
                c = BE.cut(sc, F, ms)
                if c is not None:
                    assert c["t"] >= ms
                    cuts.setdefault(c["t"], set()).add((F, ms, l, c["quota"] < len(c["ties"])))
    assert set(cuts) == {1, 2, 3}
    # with cap = 1024 thread 0 owns the scores {0, 1} and thread 1 {2, 3}: the cut on the first score of a segment (2), on
    # the last (1 and 3), with min_score = 1 or 2 inside the segment of the cutting thread, ties dropped and not
    for t, ms in ((1, 1), (2, 2), (3, 2), (3, 0), (1, 0)):
        assert any(m == ms for _, m, _, _ in cuts[t]), (t, ms)
    assert any(d for _, _, _, d in cuts[3]) and any(d for _, _, _, d in cuts[2]) and any(d for _, _, _, d in cuts[1])
    for cap in BE.SEG_CAPS:                                                    # every cap counts the same three points
        c = BE.RAW[f"seg_cap{cap}_f200_ms1"]
        assert c["cap"] == cap and c["n_dev"] == 3 and len(BE.counted(c)) == 3
    # the last bin: the score equals cap.  49 of the 81 leaves have it (the points span 3 x 3 cells of the 9 x 9), so a
    # frontier of 64 cuts below the bin with the 49 among those above the cut, and one of 32 cuts in the bin itself and drops ties
    ref, c = BE.reference("seg_last_bin"), BE.RAW["seg_last_bin"]
    assert c["cap"] == c["n_dev"] == 1024 and c["kw"]["frontier"] == 64
    assert ref["candidates"].tolist() == [81, 25, 9] and ref["kept"].tolist() == [64, 25, 9]
    assert ref["score"].tolist() == [1024] * 8 and [int(s.max()) for s in ref["slot_scores"]] == [1024] * 3
    p = BE.cut(ref["slot_scores"][0], 64)
    assert 0 < p["t"] < 1024 and p["above"] >= 49 == int((ref["slot_scores"][0] == c["cap"]).sum())
    ref, c = BE.reference("seg_last_bin_f32"), BE.RAW["seg_last_bin_f32"]
    p = BE.cut(ref["slot_scores"][0], 32)
    assert p["t"] == 1024 == c["cap"] and p["above"] == 0 and p["quota"] == 32 < len(p["ties"]) == 49
    assert ref["dropped_bound"] == 1024 and ref["certified"] == 0 and ref["kept"].tolist() == [32, 25, 9]


def test_the_far_cases_reach_the_storage_limit_with_every_sign():
    """k_bbs_offsets / k_bbs_score: (dy << 16) | (dx & 0xFFFF), (short), >> 16, abs(d) < BBS_MAX_STORE"""
    for key, (H, W, L) in (("far_w_l3", (1, 16377, 3)), ("far_h_l3", (16377, 1, 3)), ("far_w_l0", (1, 16384, 0))):
        g = BE.GRIDS[key]
        assert g["G0"].shape == (H, W) and g["L"] == L and max(H, W) + (1 << L) - 1 == BE.MAX_STORE
        assert g["G0"].reshape(-1)[0] == 1 and g["G0"].reshape(-1)[16376] == 1 and (g["i0"], g["j0"]) != (0, 0)
    cs = BR.yaw_table(4)
    for axis, key in ((0, "far_w_l3"), (1, "far_h_l3")):
        offs, n = BR.offsets(BE.far_points(axis), np.eye(4), BI.SCAN_Z, BE.R, cs)
        assert n == 18
        long0, short0 = offs[0][axis], offs[0][1 - axis]                       # yaw 0: the offsets as listed, the other axis 0
        assert sorted(set(long0.tolist())) == sorted(c for c, _ in BE.FAR_POINTS) and not short0.any()
        pairs = {(int(x), int(y)) for a in range(4) for x, y in zip(*offs[a])}
        big = 16370
        assert any(x >= big for x, y in pairs) and any(x <= -big for x, y in pairs)
        assert any(y >= big for x, y in pairs) and any(y <= -big for x, y in pairs)
        assert any(abs(x) == 16383 for x, y in pairs) and any(abs(y) == 16383 for x, y in pairs)       # legal, out of reach
        assert any(abs(x) >= 16384 for x, y in pairs) and any(abs(y) >= 16384 for x, y in pairs)       # void
        assert any(x == -1 and abs(y) >= big for x, y in pairs) and any(y == -1 and abs(x) >= big for x, y in pairs)
        # the best leaf at yaw 0 needs the +16376 hit; at pi the best leaf of the wide grid needs the -16376 hit (the points of
        # offset 16375 turned round), that of the tall grid the +16374 hit (the point of offset -16375)
        ex = BE.exhaustive(f"{key}_a2")
        for a, far in ((0, 16376), (1, 16375 if axis == 0 else -16375)):
            less = BR.exhaustive(BE.GRIDS[key]["G0"], BE.R, BE.far_points(axis, (far,)), 2, scan_z=BI.SCAN_Z)
            assert less[a].max() < ex[a].max(), (key, a)
        d = offs[2][axis][long0.tolist().index(16375 if axis == 0 else -16375)]
        assert d == (-16376 if axis == 0 else 16374)
        ref = BE.reference(f"{key}_a4")
        assert (ref["kept"] == 4096).all() and (ref["candidates"] > 8000).all() and ref["certified"] == 8   # cut at every level
        leaf = 16376 if axis == 0 else 0                                      # the best leaf of yaw pi, id (a * H + j) * W + i
        assert ref["index"][0] == 0 and ref["score"][0] == 7 and int(ex[1].argmax()) == leaf
    ref = BE.reference("far_w_l0_a2")
    assert ref["candidates"].tolist() == [32768] and ref["kept"].tolist() == [8192]
    # level 7 of 130 x 130: the root nodes at i = 0 score through pooled cells at x = -127 .. -1
    c, g = BE.RAW["pad_l7"], BE.GRIDS["pad_l7"]
    assert g["G0"].shape == (130, 130) and g["L"] == 7
    offs, _ = BR.offsets(c["pts"], np.eye(4), BI.SCAN_Z, BE.R, BR.yaw_table(c["A"]))
    G7 = BR.pooled(g["G0"], 7)
    for a, (dx, dy) in enumerate(offs):
        neg = (dx >= -127) & (dx <= -1)
        assert neg.sum() > 20 and BR.lookup(G7, 7, dx[neg], dy[neg]).sum() > 0 and dx[neg].min() < -100
    assert BE.reference("pad_l7")["candidates"][7] == 12


def test_the_count_and_frontier_cases_sit_on_their_limits():
    """n = min(cap, max(*n_dev, 0)); frontier 1 and SPS_BBS_MAX_FRONTIER"""
    at, beyond = BE.RAW["count_at_cap"], BE.RAW["count_beyond_cap"]
    assert at["n_dev"] == at["cap"] == 256 and beyond["n_dev"] == beyond["cap"] + 1000 and len(beyond["pts"]) > beyond["cap"]
    assert BE.RAW["count_negative"]["n_dev"] == -5 and BE.RAW["count_zero"]["n_dev"] == 0
    a, b = BE.reference("count_at_cap"), BE.reference("count_beyond_cap")
    assert a["n_slice"] == b["n_slice"] == 256 and a["index"].tolist() == b["index"].tolist() and a["certified"] == 8
    for n in ("count_zero", "count_negative"):
        assert BE.reference(n)["n_slice"] == 0 and BE.reference(n)["n_found"] == 0
    one = BE.reference("frontier_1")
    assert BE.RAW["frontier_1"]["A"] == 4 and one["candidates"][3] == 4 and one["kept"][3] == 1 and one["dropped_bound"] > 0
    assert BE.reference("frontier_1_min_score_0")["n_found"] == 1
    big = BE.reference("frontier_65536")
    assert BE.RAW["frontier_65536"]["kw"]["frontier"] == 65536 and big["candidates"][0] > 12 * BE.SCAN_BLOCK and big["certified"] == 8
