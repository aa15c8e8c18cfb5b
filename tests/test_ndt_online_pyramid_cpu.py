"""CPU tests of the online NDT pyramid's numpy restatement (tests/ndt_online_pyramid_reference.py), of the binding, of the
constructor's checks and of the driver's options.  No GPU.  The scene is tests/test_ndt_carve_cpu.py's phantom scene (the
synthetic map plus a 1 500-point pole that no scan sees) at 2 / 1 / 0.5 m, the scans tests/test_ndt_cpu.py's, thinned at leaf
0.4 (about 4 157 points)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_online_pyramid_reference as OP
from tests import ndt_pyramid_reference as PR
from tests import ndt_reference as NR
from tests.test_ndt_carve_cpu import phantom_pole, thinned
from tests.test_ndt_cpu import KW, T_TRUE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOLUTIONS = (2.0, 1.0, 0.5)
CAPACITIES = (2048, 4096, 16384)
# info words (rays, seen through, cleared, cut) per frame and level, default carve options: the restatement's own output
PHANTOM_INFO = {
    1: ([4157, 2, 0, 0], [4157, 2, 0, 0], [4157, 14, 0, 0]),
    2: ([4152, 2, 0, 0], [4152, 2, 0, 0], [4152, 14, 0, 0]),
    3: ([4156, 1, 1, 0], [4156, 2, 2, 0], [4156, 14, 14, 0]),
}
PHANTOM_CELLS = (841, 2535, 7799)                                    # cells of the scene per level
PHANTOM_ONLY = (1, 2, 16)                                            # of them, cells that only the pole fills
FIELDS = ("count", "mean", "icov", "valid", "S")


def phantom_pyramid_scene():
    """(the map's points with the phantom pole, per level the ids of the cells that only the phantom fills)"""
    mp = synthetic.build_map(**KW)[:, :3].astype(np.float64)
    with_pole = np.concatenate([mp, phantom_pole()])
    only = []
    for r in RESOLUTIONS:
        have = set(int(k) for k in NR.group(mp, r)[0])
        only.append(np.array([i for i, k in enumerate(NR.group(with_pole, r)[0]) if int(k) not in have]))
    return with_pole, only


# ---- the phantom scene at three resolutions ------------------------------------------------------------------------------
def test_three_frames_clear_the_phantom_at_every_level_and_nothing_else_ever():
    """The condition: at no level is a cell that exists without the pole ever cleared.  At 2 m one real cell is seen through
    in frames 1 and 2 and escapes because it is not seen through in frame 3: a known margin of the defaults at coarse
    levels, counted here and not tuned away."""
    with_pole, only = phantom_pyramid_scene()
    levels = OP.build(with_pole, RESOLUTIONS, CAPACITIES)
    assert tuple(len(m["keys"]) for m in levels) == PHANTOM_CELLS and tuple(len(o) for o in only) == PHANTOM_ONLY
    assert (int(levels[0]["valid"].sum()), int(levels[2]["valid"].sum())) == (444, 3012)
    others = [np.setdiff1d(np.arange(len(m["keys"])), o) for m, o in zip(levels, only)]
    start = [{k: np.array(m[k]).copy() for k in FIELDS} for m in levels]
    for frame in (1, 2, 3):
        visited = []
        pts = thinned(frame)
        info = OP.carve(levels, pts, T_TRUE, visited=visited)
        for l, m in enumerate(levels):
            false_candidates = int((m["miss"][others[l]] > 0).sum())
            print(f"frame {frame} level {l} ({RESOLUTIONS[l]} m): info {info[l]}, cells per ray {np.mean(visited[l]):.1f} "
                  f"(most {max(visited[l])}), real cells with a miss {false_candidates}")
            assert info[l] == PHANTOM_INFO[frame][l], (frame, l)
            for k, a in start[l].items():                            # no cell that exists without the pole changes, ever
                assert np.array(m[k])[others[l]].tobytes() == a[others[l]].tobytes(), (frame, l, k)
            if l == 0:
                assert false_candidates == (0 if frame == 3 else 1)  # the margin at 2 m
            else:
                assert false_candidates == 0
    assert [int((m["count"][o] == 0).sum()) for m, o in zip(levels, only)] == [1, 2, 14]
    assert max(visited[2]) == 142 and abs(np.mean(visited[2]) - 35.4) < 0.05


def test_a_level_is_the_single_map_of_its_resolution():
    """the composition adds nothing: carve and update of level l are CR.carve / UR.update on a map built alone"""
    from tests import ndt_carve_reference as CR
    from tests import ndt_update_reference as UR
    with_pole, _ = phantom_pyramid_scene()
    mp = with_pole[::5]
    levels = OP.build(mp, RESOLUTIONS, CAPACITIES)
    pts = thinned(1)
    margins = (3.0, 1.0, 0.25)
    ci = OP.carve(levels, pts, T_TRUE, end_margin=margins, min_pass=1, miss_frames=1)
    ui = OP.update(levels, pts, T_TRUE, max_cell_points=20)
    for l, (r, c) in enumerate(zip(RESOLUTIONS, CAPACITIES)):
        m = UR.build(mp, c, r)
        assert CR.carve(m, pts, T_TRUE, end_margin=margins[l], min_pass=1, miss_frames=1) == ci[l] and ci[l][2] > 0
        assert UR.update(m, pts, T_TRUE, max_cell_points=20) == ui[l]
        for k in ("keys",) + FIELDS + ("pass", "hit", "miss"):
            assert np.array(m[k]).tobytes() == np.array(levels[l][k]).tobytes(), (l, k)
    assert OP.margins(levels) == list(RESOLUTIONS) and OP.margins(levels, 0.5) == [0.5] * 3
    # a closed gate: no byte of any level, info (assigned, 0, 0, 0) and zeros
    for m in levels:
        CR.state(m)                                                          # the founded cells' counters, zero
    before = [{k: np.array(m[k]).copy() for k in ("keys",) + FIELDS + ("pass", "hit", "miss")} for m in levels]
    assert OP.update(levels, pts, T_TRUE, gate=2) == [[len(m["keys"]), 0, 0, 0] for m in levels]
    assert OP.carve(levels, pts, T_TRUE, gate=2) == [[0, 0, 0, 0]] * 3
    for m, b in zip(levels, before):
        for k, a in b.items():
            assert np.array(m[k]).tobytes() == a.tobytes(), k


def test_an_empty_pyramid_plus_one_update_equals_the_static_pyramid():
    pts = thinned(2)
    q = LR.transform(pts, T_TRUE)
    levels = OP.build(np.zeros((0, 3)), RESOLUTIONS, CAPACITIES)
    assert [len(m["keys"]) for m in levels] == [0, 0, 0]
    info = OP.update(levels, pts, T_TRUE)
    want = PR.pyramid(q, RESOLUTIONS)
    for l, (got, w) in enumerate(zip(OP.cmaps(levels), want)):
        assert info[l] == [len(w["keys"]), len(w["keys"]), 0, len(pts)] and len(w["keys"]) > 100
        for k in ("keys", "count", "mean", "icov", "valid"):
            a, b = np.asarray(got[k]), np.asarray(w[k])
            assert a.shape == b.shape and a.astype(b.dtype).tobytes() == b.tobytes(), (l, k)
    assert [int(w["valid"].sum()) for w in want][1] > 50
    # and the alignment runs on the levels as they are now (a budget that ends before the 0.5 m level, whose cells hold
    # too few of one thinned scan's points to be valid)
    r = OP.align(pts, levels, T_TRUE, iters=4, level_iters=(2, 2, 2))
    assert r["status"] in (0, 1) and r["n_corr"] > 1000 and r["level"] == 1


# ---- the binding, the constructor, the driver ------------------------------------------------------------------------------
def test_the_binding_knows_the_online_pyramid_entry_points():
    from sps_amd import _native
    for name in ("sps_ndt_pyramid_build_dynamic", "sps_ndt_pyramid_update_scratch", "sps_ndt_pyramid_update",
                 "sps_ndt_pyramid_carve_scratch", "sps_ndt_pyramid_carve", "sps_ndt_pyramid_info", "sps_ndt_pyramid_carve_cells"):
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
    assert _native.lib.sps_version() == _native.ABI_VERSION == 202           # additive: the ABI version does not change
    one = _native.lib.sps_ndt_map_update_scratch
    many = _native.lib.sps_ndt_pyramid_update_scratch
    assert many(1000, 1) == one(1000)                                        # one level: the single map's layout
    q = (1000 * 24 + 255) // 256 * 256                                       # the points, stored once for all levels
    assert one(1000) < many(1000, 3) <= 3 * one(1000) - 2 * q
    assert many(65537, 3) == -1 and many(-1, 3) == -1 and many(1000, 0) == -1 and many(1000, 5) == -1
    carve = _native.lib.sps_ndt_pyramid_carve_scratch
    assert carve(65536, 4) == 0 and carve(65537, 4) == -1 and carve(10, 0) == -1
    for name in ("ndt_pyramid_update", "ndt_pyramid_carve", "ndt_pyramid_info", "ndt_pyramid_carve_cells"):
        assert callable(getattr(_native.Context, name))


def test_constructor_errors_come_before_any_device_work():
    """device="nowhere:0" is never looked at: every one of these is refused first"""
    from sps_amd.localiser import MAX_UPDATE_POINTS, NDTLocaliser
    mp = np.stack(np.meshgrid(*[np.arange(4) + 0.5] * 3, indexing="ij"), axis=-1).reshape(-1, 3)   # 8 cells of 2 m, 64 of 1 m
    for kw in (dict(level_capacities=(64,)),                                                   # no pyramid
               dict(resolutions=(2.0, 1.0), level_capacities=(64,)),                          # the wrong length
               dict(resolutions=(2.0, 1.0), level_capacities=(64, 64, 64)),
               dict(resolutions=(2.0, 1.0), level_capacities=(0, 64)),                        # an entry below 1
               dict(resolutions=(2.0, 1.0), level_capacities=(7, 64)),                        # below the level's 8 cells
               dict(resolutions=(2.0, 1.0), level_capacities=(8, 63)),                        # below the level's 64 cells
               dict(resolutions=(2.0, 1.0), level_capacities=(64, 64), cell_capacity=64),     # the single map stays static
               dict(resolutions=(2.0, 1.0), level_capacities=(64, 64), capacity=MAX_UPDATE_POINTS + 1)):
        with pytest.raises(ValueError):
            NDTLocaliser(mp, device="nowhere:0", **kw)
    assert NDTLocaliser._checked_level_capacities((2.0, 1.0), (8, 64), 1000, mp) == (8, 64)
    assert NDTLocaliser._checked_level_capacities((2.0, 1.0), (1, 1), 1000, np.zeros((0, 3))) == (1, 1)
    assert NDTLocaliser._checked_level_capacities(None, None, 1 << 20, mp) is None
    with pytest.raises(ValueError, match="single-resolution"):               # pinned: still refused as before
        NDTLocaliser(mp, device="nowhere:0", resolutions=(2.0, 1.0), cell_capacity=64)


def test_the_checks_on_bare_objects():
    from sps_amd.localiser import NDTLocaliser
    # a pyramid without level_capacities: as before (the attribute may be missing altogether)
    loc = object.__new__(NDTLocaliser)
    loc.resolutions, loc.cell_capacity = (2.0, 1.0), None
    with pytest.raises(ValueError, match="single-resolution"):
        loc._check_integrate(True)
    with pytest.raises(ValueError, match="single-resolution"):
        loc._check_carve(True)
    # a static single map: as before
    loc = object.__new__(NDTLocaliser)
    loc.resolutions, loc.cell_capacity = None, None
    with pytest.raises(ValueError, match="online map"):
        loc._check_integrate(True)
    with pytest.raises(ValueError, match="online map"):
        loc._check_carve(True)
    # an online pyramid
    loc = object.__new__(NDTLocaliser)
    loc.resolutions, loc.cell_capacity, loc.level_capacities, loc.resolution = (2.0, 1.0), None, (64, 64), 1.0
    loc._check_integrate(True)
    with pytest.raises(ValueError):
        loc._check_integrate(True, max_cell_points=-1)
    assert loc._check_carve(True)["end_margin"] == (2.0, 1.0)                # None: each level's resolution
    assert loc._check_carve(True, dict(end_margin=0.5))["end_margin"] == (0.5, 0.5)
    assert loc._check_carve(True, dict(end_margin=[3, 0.25]))["end_margin"] == (3.0, 0.25)
    for bad in (dict(end_margin=(1.0,)), dict(end_margin=(1.0, -1.0)), dict(end_margin=(1.0, float("inf"))), dict(max_steps=0)):
        with pytest.raises(ValueError):
            loc._check_carve(True, bad)
    # the single map beside it is static: what the batch and the search ask
    with pytest.raises(ValueError, match="online map"):
        loc._check_integrate(True, single_map=True)
    with pytest.raises(ValueError, match="online map"):
        loc._check_carve(True, single_map=True)
    with pytest.raises(ValueError, match="online map"):
        loc.submit_batch(None, 0, np.eye(4)[None], integrate=True)
    with pytest.raises(ValueError, match="online map"):
        loc.relocalise(None, 0, np.eye(4)[None], carve=True)
    with pytest.raises(ValueError):
        loc.carve_state()                                                    # the single map has no carve state
    with pytest.raises(ValueError):
        loc.carve_state(2)
    with pytest.raises(ValueError):
        loc.pyramid_info(-1)


def test_results_come_per_level():
    from sps_amd.localiser import MapCarveResult, MapUpdateResult, _map_carve_of, _map_update_of, _per_level
    words = np.arange(12, dtype=np.int32)
    assert _per_level(_map_update_of, words, 9, None) == MapUpdateResult(0, 1, 2, 3, 9)
    assert _per_level(_map_carve_of, words, 9, 3) == (MapCarveResult(0, 1, 2, 3, 9), MapCarveResult(4, 5, 6, 7, 9),
                                                       MapCarveResult(8, 9, 10, 11, 9))


def test_the_driver_lists_the_online_pyramid_options():
    script = os.path.join(ROOT, "scripts", "filter_sequence.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-1500:]
    assert "--level-capacities" in r.stdout
    cmd = [sys.executable, script, "--synthetic", "2", "--localise", "--localiser", "ndt", "--update-map", "--level-capacities", "64,64"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--level-capacities needs --resolutions" in r.stderr
