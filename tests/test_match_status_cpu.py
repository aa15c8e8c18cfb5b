"""CPU tests of the scan-matching status: the numpy restatement (tests/match_status_reference.py) against a KD-tree, its
verdict table, the figures the GPU tests' threshold rests on, the option checks and the loop's policy with stub stages.
No GPU."""
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest

from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import match_status_reference as MR
from tests import ndt_reference as NR

KW = dict(n_azimuth=400, n_beams=32)
T_TRUE = LR.perturbation(0.8, -0.3, 0.05, 20.0)
T_INIT = LR.perturbation(0.2, 0.2, 0.1, 2.0) @ T_TRUE
THRESHOLD = 0.85                                        # min_inlier_fraction of the GPU tests
# the starts of the table: (dx, dy, yaw in degrees) of T_TRUE @ perturbation(dx, dy, 0, yaw), and what was measured
LOST_STARTS = [((10.0, 0.0, 0.0), 0.2307), ((0.0, 0.0, 90.0), 0.2379), ((20.0, 0.0, 180.0), 0.1706), ((3.0, 0.0, 0.0), 0.7125),
               ((0.0, 3.0, 0.0), 0.2668), ((0.0, 1.0, 10.0), 0.4280)]


def sensor_scan(seed, T_true=T_TRUE):
    world = synthetic.lidar_scan(seed, **KW)
    Ti = np.linalg.inv(T_true)
    xyz = world[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]
    return np.c_[xyz, world[:, 3]].astype(np.float32)


@pytest.fixture(scope="module")
def scene():
    scan = sensor_scan(1)
    map_xyz = synthetic.build_map(**KW)[:, :3].astype(np.float64)
    from scipy.spatial import cKDTree
    return dict(map=map_xyz, pts=LR.downsample(scan, len(scan), 0.4)[1], cmap=NR.cells(map_xyz, 1.0), tree=cKDTree(map_xyz))


def test_the_restatement_finds_the_kd_trees_neighbour(scene):
    from scipy.spatial import cKDTree
    pts, m = scene["pts"], scene["map"]
    assert len(pts) == 4157
    q = MR.transform(pts, T_TRUE)
    d2, j = MR.nearest(q, m, 0.5)
    dist, k = cKDTree(m).query(q, k=2)
    # the tree's distance is a square root; compare at 4 ulp of the squared distance (the square doubles a relative error)
    np.testing.assert_allclose(d2, dist[:, 0] ** 2, rtol=4 * 2.0 ** -52, atol=0)
    unique = dist[:, 0] < dist[:, 1]
    assert unique.sum() > 0.99 * len(pts)
    np.testing.assert_array_equal(j[unique], k[unique, 0])
    # the narrowed search the larger tests use gives the brute-force search's inliers, bit for bit
    for r in (0.5, 0.05):
        d2n, jn = MR.nearest_within(q, m, 0.5, r, scene["tree"])
        inl = d2 <= r * r
        assert 0 < inl.sum() and np.array_equal(jn >= 0, inl)
        assert np.array_equal(d2n[inl], d2[inl]) and np.array_equal(jn[inl], j[inl]) and np.isinf(d2n[~inl]).all()
    e = q - m[j]                                                           # the d2 is the kernel's expression at that point
    np.testing.assert_array_equal(d2, (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    # ties go to the lowest map index
    twin = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    d2t, jt = MR.nearest(np.zeros((1, 3)), twin, 2.0)
    assert d2t[0] == 1.0 and jt[0] == 0
    d2t, jt = MR.nearest(np.zeros((1, 3)), twin[::-1].copy(), 2.0)
    assert jt[0] == 0
    # no neighbour: an empty map, a q that is not finite, a q beyond the key range
    assert MR.nearest(np.zeros((1, 3)), np.zeros((0, 3)), 0.5)[1][0] == -1
    far = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0.5 * 1048576.0, 0, 0], [0.5 * 1048575.0, 0, 0]])
    assert MR.nearest(far, twin, 0.5)[1].tolist() == [-1, -1, -1, 0]


def test_the_two_stage_sum_adds_in_the_devices_order():
    rng = np.random.default_rng(5)
    n = 9 * 32 + 1
    v = rng.uniform(0.0, 1.0, n) * 10.0 ** rng.integers(-8, 8, n)
    inl = rng.uniform(size=n) < 0.7
    rows = []
    for b in range(10):
        s = 0.0
        for i in range(32 * b, min(n, 32 * b + 32)):
            s = s + (v[i] if inl[i] else 0.0)
        rows.append(s)
    runs = [rows[2 * g] + rows[2 * g + 1] for g in range(5)]               # 10 rows: five runs of two, three empty ones
    want = (((runs[0] + runs[1]) + runs[2]) + runs[3]) + runs[4]
    assert MR.two_stage_sum(v, inl, n) == want
    assert MR.two_stage_sum(v, inl, 0) == 0.0
    assert abs(want - math.fsum(v[inl])) <= 1e-12 * math.fsum(v[inl])


@pytest.mark.parametrize("gate_in", [None, 0, 1, 2, 3, -1])
def test_the_verdict_table(gate_in):
    opts = dict(min_inlier_fraction=0.5, max_error=0.1, min_valid=10)
    good = dict(n_valid=10, fraction=0.5, error=0.1)                       # each threshold met exactly
    bad = dict(n_valid=9, fraction=np.nextafter(0.5, 0.0), error=np.nextafter(0.1, 1.0))
    for fails in itertools.product((False, True), repeat=3):
        kw = {k: (bad if f else good)[k] for k, f in zip(("n_valid", "fraction", "error"), fails)}
        got = MR.verdict(gate_in, **kw, **opts)
        if gate_in in (2, 3, -1):
            assert got == gate_in                                         # the registration had failed already
        else:
            assert got == (MR.LOST if any(fails) else (gate_in or 0))
    # no inliers: the error is inf, which only max_error = inf lets pass
    assert MR.verdict(gate_in, 5, 0.0, math.inf, 0.0, math.inf, 1) == (0 if gate_in is None else gate_in)
    if gate_in in (None, 0, 1):
        assert MR.verdict(gate_in, 5, 0.0, math.inf, 0.0, 1e300, 1) == MR.LOST


def test_the_status_of_a_small_case_by_hand():
    m = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    pts = np.array([[0.25, 0.0, 0.0], [0.5, 0.0, 0.0], [3.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [1.0, 0.25, 0.0], [9.0, 9.0, 9.0]])
    r = MR.status(pts, 5, 6, np.eye(4), m, 0.5, max_distance=0.5, min_inlier_fraction=0.75)
    assert (r["n"], r["n_valid"], r["n_inliers"]) == (5, 4, 3)
    assert r["d2"].tolist() == [0.0625, 0.25, math.inf, -1.0, 0.0625] and r["j"].tolist() == [0, 0, -1, -1, 1]
    assert r["sum_d2"] == 0.375 and r["inlier_fraction"] == 0.75 and r["matching_error"] == 0.125 and r["verdict"] == 0
    assert MR.status(pts, 5, 6, np.eye(4), m, 0.5, min_inlier_fraction=0.76)["verdict"] == MR.LOST
    assert MR.status(pts, 5, 6, np.eye(4), m, 0.5, min_inlier_fraction=0.76, gate_in=3)["verdict"] == 3
    r = MR.status(pts, 9, 6, np.eye(4), m, 0.5, max_range=1.0)              # n_dev > cap; (1, 0.25, 0) is out of range
    assert (r["n"], r["n_valid"], r["n_inliers"]) == (6, 2, 2) and r["d2"].tolist() == [0.0625, 0.25, -1.0, -1.0, -1.0, -1.0]
    r = MR.status(pts, -3, 6, np.eye(4), m, 0.5)
    assert (r["n"], r["n_valid"], r["inlier_fraction"], r["matching_error"], r["verdict"]) == (0, 0, 0.0, math.inf, MR.LOST)
    assert len(MR.out_bytes(r)) == 48


def test_the_inlier_fraction_separates_the_lost_registrations(scene):
    """The condition the GPU tests' threshold (0.85) rests on: the table of measurements that motivated the status, from the
    restatements alone.  Printed: start, NDT status, error at the end pose, inlier fraction there."""
    pts, m, cmap = scene["pts"], scene["map"], scene["cmap"]

    def run(T0):
        r = NR.align(pts, cmap, T0, iters=30)
        s = MR.status(pts, len(pts), len(pts), r["pose"], m, 0.5, tree=scene["tree"])
        dt, dr = LR.pose_difference(r["pose"], T_TRUE)
        return r["status"], dt, dr, s

    st, dt, dr, s = run(T_INIT)
    print(f"T_INIT: status {st}, {dt:.3f} m {dr:.4f} rad, fraction {s['inlier_fraction']:.4f}, error {s['matching_error']:.5f}")
    assert st == 0 and dt < 0.05 and s["inlier_fraction"] > THRESHOLD
    assert s["inlier_fraction"] == 1.0 and s["n_valid"] == len(pts)
    worst = 0.0
    for (dx, dy, yaw), measured in LOST_STARTS:
        st, dt, dr, s = run(T_TRUE @ LR.perturbation(dx, dy, 0.0, yaw))
        print(f"({dx}, {dy}, {yaw}): status {st}, {dt:.3f} m {dr:.4f} rad, fraction {s['inlier_fraction']:.4f} "
              f"(measured {measured})")
        assert st in (0, 1) and (dt > 0.5 or dr > 0.1)                     # the registration's own status lets it pass
        assert abs(s["inlier_fraction"] - measured) < 5e-4                 # the table, to the digits it gives
        worst = max(worst, s["inlier_fraction"])
    assert worst <= 0.7125 + 5e-5 and worst < THRESHOLD


def test_match_status_options_are_checked_before_any_device_work():
    from sps_amd.localiser import MATCH_DEFAULTS, _checked_match, LOST, STATUS_NAMES
    assert LOST == 4 == MR.LOST and LOST in STATUS_NAMES
    assert _checked_match(None) is None
    assert _checked_match({}) == MATCH_DEFAULTS == dict(max_distance=0.5, max_range=None, min_inlier_fraction=0.0,
                                                         max_error=math.inf, min_valid=1)
    assert _checked_match(dict(max_range=30, min_valid=5))["max_range"] == 30.0
    for bad in (dict(radius=1.0), dict(max_distance=0.0), dict(max_distance=math.inf), dict(max_distance=math.nan),
                dict(max_distance="x"), dict(max_range=-1.0), dict(max_range=math.nan), dict(min_inlier_fraction=math.nan),
                dict(min_inlier_fraction=1.5), dict(max_error=math.nan), dict(max_error=-1.0), dict(min_valid=-1),
                dict(min_valid=1.5)):
        with pytest.raises(ValueError):
            _checked_match(bad)


def test_the_layouts_grow_by_six_words_only_with_a_status():
    from sps_amd.localiser import _batch_layout, _pose_layout
    for args in ((30, False), (5, True, True, 3, True, True)):
        a, b = _pose_layout(*args), _pose_layout(*args, match=True)
        assert b["total"] == a["total"] + 6 and b["match"] == a["total"] == a["match"]
        assert a["hands_on"] == (0, a["status"] * 8) and b["hands_on"] == (0, (b["match"] + 4) * 8)
        assert {k: v for k, v in a.items() if k not in ("hands_on", "total")} == {k: v for k, v in b.items()
                                                                                  if k not in ("hands_on", "total")}
    for args in ((4, 30, False), (2, 5, True, True, True, True, 3)):
        a, b = _batch_layout(*args), _batch_layout(*args, match=True)
        assert b["total"] == a["total"] + 6 and b["match"] == a["total"]
        assert a["hands_on"] == (a["T_best"] * 8, a["best"] * 8 + 4) and b["hands_on"] == (a["T_best"] * 8, (b["match"] + 4) * 8)


def test_the_binding_knows_the_entry_points():
    from sps_amd import _native
    for name in ("sps_loc_match_status_scratch", "sps_loc_match_status"):
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
    assert _native.lib.sps_version() == _native.ABI_VERSION                 # additive: the ABI version does not change
    assert _native.lib.sps_loc_match_status_scratch(0) == 32 and _native.lib.sps_loc_match_status_scratch(33) == 48
    assert _native.lib.sps_loc_match_status_scratch(-1) == -1


# ---- the loop's policy with stub stages -----------------------------------------------------------------------------------
class _Pending:
    def __init__(self, res):
        self._res = res

    def result(self):
        return self._res


class _Filter:
    def submit(self, scan, pose):
        return _Pending(SimpleNamespace(filtered=scan[:3]))


def _match(lost):
    return SimpleNamespace(lost=lost, verdict=4 if lost else 0, inlier_fraction=0.2 if lost else 1.0)


class _Localiser:
    """``submit`` answers shift @ guess, lost at the frames of ``lost_at`` (frames counted over both entry points);
    ``localise_global`` answers ``found``, selected and matching except at the frames of ``global_fails``: there, by turns,
    nothing selected and selected but lost."""
    device = "cpu"
    _global = dict(levels=3)

    def __init__(self, shift, found, lost_at=(), global_fails=()):
        self.shift, self.found, self.lost_at, self.global_fails = shift, found, set(lost_at), list(global_fails)
        self.calls = []

    def submit(self, rows, count, T_init):
        k = len(self.calls)
        self.calls.append(("submit", np.array(T_init)))
        return _Pending(SimpleNamespace(pose=self.shift @ np.array(T_init), status=1 if k in self.lost_at else 0,
                                        match=_match(k in self.lost_at)))

    def localise_global(self, rows, count, yaw_steps, **kw):
        k = len(self.calls)
        self.calls.append(("global", yaw_steps, kw))
        fail = self.global_fails.index(k) if k in self.global_fails else -1
        best = -1 if fail >= 0 and fail % 2 == 0 else 0
        batch = SimpleNamespace(best=best, results=[SimpleNamespace(pose=self.found, status=0)], match=_match(fail >= 0 and best == 0),
                                pose=self.found)
        return _Pending(SimpleNamespace(index=7 if best == 0 else -1, pose=self.found, batch=batch))


def test_the_loop_recovers_globally_after_two_flagged_frames():
    from sps_amd.localiser import LocalisationLoop
    shift = LR.perturbation(0.5, 0.0, 0.0, 1.0)
    found = LR.perturbation(40.0, 3.0, 0.0, 120.0)
    T0 = LR.perturbation(2.0, 1.0, 0.0, 10.0)
    scan = np.zeros((5, 4), dtype=np.float32)
    # frames 0..4 fill the model; 5 and 6 are lost; 7 and 8 search and fail (none selected, then selected but lost); 9 recovers
    loc = _Localiser(shift, found, lost_at=(5, 6), global_fails=(7, 8))
    loop = LocalisationLoop(_Filter(), loc, T0, recover=dict(after=2, yaw_steps=72, keep=4, frontier=1000))
    steps = [loop.step(scan) for _ in range(12)]
    assert [c[0] for c in loc.calls] == ["submit"] * 7 + ["global"] * 3 + ["submit"] * 2
    assert loc.calls[7][1] == 72 and loc.calls[7][2] == dict(keep=4, frontier=1000, min_score=1, scan_z=None, T_up=None)
    assert [s.flagged for s in steps] == [False] * 5 + [True] * 4 + [False] * 3
    assert [s.recovered for s in steps] == [False] * 9 + [True] + [False] * 2
    assert [s.match.lost for s in steps] == [False] * 5 + [True, True, False, True] + [False] * 3
    for k in (5, 6, 7, 8):                                                 # a flagged frame keeps the guess
        np.testing.assert_array_equal(steps[k].pose, steps[k].guess)
    assert steps[7].global_result is not None and steps[6].global_result is None
    np.testing.assert_array_equal(steps[9].pose, found)
    # the model was emptied: it held nine poses, now the recovered one and what followed; the next guess is the last pose,
    # not a constant-velocity prediction across the jump
    assert len(loop.model.poses) == 3
    np.testing.assert_array_equal(loop.model.poses[0], found)
    np.testing.assert_array_equal(steps[10].guess, found)
    np.testing.assert_array_equal(steps[11].guess, steps[10].pose)
    assert len(loop.poses) == 12


def test_one_lost_frame_does_not_start_a_recovery_after_two():
    from sps_amd.localiser import LocalisationLoop
    shift = LR.perturbation(0.5, 0.0, 0.0, 1.0)
    loc = _Localiser(shift, np.eye(4), lost_at=(1, 3))
    loop = LocalisationLoop(_Filter(), loc, np.eye(4), recover=dict(after=2, yaw_steps=8))
    steps = [loop.step(np.zeros((5, 4), dtype=np.float32)) for _ in range(5)]
    assert [c[0] for c in loc.calls] == ["submit"] * 5 and [s.flagged for s in steps] == [False, True, False, True, False]


def test_recover_is_checked():
    from sps_amd.localiser import LocalisationLoop
    loc = _Localiser(np.eye(4), np.eye(4))
    for bad in (dict(yaw_steps=8), dict(after=0, yaw_steps=8), dict(after=1), dict(after=1, yaw_steps=8, radius=2)):
        with pytest.raises(ValueError):
            LocalisationLoop(_Filter(), loc, np.eye(4), recover=bad)
    no_grid = SimpleNamespace(device="cpu", submit=None)
    with pytest.raises(ValueError):
        LocalisationLoop(_Filter(), no_grid, np.eye(4), recover=dict(after=1, yaw_steps=8))
    est = SimpleNamespace(predict=None, predict_imu=None, pose_dev=None, correct_from=None, snapshot=None)
    with pytest.raises(ValueError):
        LocalisationLoop(_Filter(), loc, np.eye(4), recover=dict(after=1, yaw_steps=8), estimator=est, device_guess=True)
    # an online pyramid that the loop updates takes no recovery on the single map, as it takes no hypotheses and no search
    pyramid = _Localiser(np.eye(4), np.eye(4))
    pyramid.resolutions, pyramid.level_capacities = (2.0, 1.0), (100, 400)
    for kw in (dict(update_map=True), dict(carve_map=True)):
        with pytest.raises(ValueError, match="online pyramid"):
            LocalisationLoop(_Filter(), pyramid, np.eye(4), recover=dict(after=1, yaw_steps=8), **kw)
        LocalisationLoop(_Filter(), pyramid, np.eye(4), recover=dict(after=1, yaw_steps=8), coarse_to_fine=True, **kw)
    LocalisationLoop(_Filter(), pyramid, np.eye(4), recover=dict(after=1, yaw_steps=8))
    # an estimator that cannot be re-initialised
    with pytest.raises(TypeError, match="reset"):
        LocalisationLoop(_Filter(), loc, np.eye(4), recover=dict(after=1, yaw_steps=8), estimator=est)
    LocalisationLoop(_Filter(), loc, np.eye(4), estimator=est)
    # a result without ``match`` (a localiser of the caller's own) is never lost
    plain = SimpleNamespace(device="cpu", submit=lambda rows, count, T: _Pending(SimpleNamespace(pose=np.array(T), status=0)))
    st = LocalisationLoop(_Filter(), plain, np.eye(4)).step(np.zeros((5, 4), dtype=np.float32))
    assert st.match is None and not st.flagged and not st.recovered
