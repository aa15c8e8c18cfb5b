"""CPU tests of the localiser's host side: the numpy restatement (tests/localiser_reference.py) on a synthetic scan, the
trajectory statistics and file format, the control flow of LocalisationLoop with stub stages, and the C ABI."""
import os
import re

import numpy as np
import pytest

from sps_amd import synthetic
from tests import localiser_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(n_azimuth=400, n_beams=32)
NOISE = 0.01                                            # synthetic.lidar_scan: Gaussian range noise, sigma = 1 cm


def sensor_scan(seed, T_true):
    world = synthetic.lidar_scan(seed, **KW)[:, :3].astype(np.float64)
    Ti = np.linalg.inv(T_true)
    return (world @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)


def test_restatement_recovers_a_known_perturbation():
    T_true = LR.perturbation(0.8, -0.3, 0.05, 20.0)
    scan = sensor_scan(1, T_true)
    _, pts = LR.downsample(scan, len(scan), 0.4)
    index = LR.MapIndex(synthetic.build_map(**KW), 1.0)
    T_init = LR.perturbation(0.2, 0.2, 0.1, 2.0) @ T_true             # 0.3 m and 2 degrees off
    d0 = LR.pose_difference(T_init, T_true)
    assert 0.25 < d0[0] < 0.35 and abs(np.degrees(d0[1]) - 2.0) < 0.1
    r = LR.align(pts, index, T_init, iters=30)
    assert r["status"] == 0 and r["iterations"] < 30
    dt, dr = LR.pose_difference(r["pose"], T_true)
    assert dt < NOISE and dr < NOISE / 10.0                           # 1 cm; 1 cm over a 10 m lever arm
    assert r["trace"][-1, 2] < 1e-4 and r["trace"][-1, 3] < 1e-5
    assert (r["trace"][:, 0] >= 50).all()
    # the b the restatement reports is minus the summed J^T e terms
    np.testing.assert_array_equal(r["normal"][0, 21:27], np.add.accumulate(r["terms"][0][:, 21:27], axis=0)[-1])


def test_restatement_downsample_keeps_the_lowest_row_of_a_voxel():
    rows = np.array([[0.05, 0.05, 0.05], [-0.05, 0.05, 0.05], [0.15, 0.1, 0.0], [0.3, 0.0, 0.0], [np.nan, 0, 0],
                     [-0.01, 0.19, 0.0], [3e6, 0, 0], [0.21, 0.01, 0.01]], dtype=np.float32)
    keep, pts = LR.downsample(rows, len(rows), 0.2)
    assert keep.tolist() == [0, 1, 3]
    assert pts.dtype == np.float64 and np.array_equal(pts, rows[[0, 1, 3]].astype(np.float64))
    assert LR.downsample(rows, 2, 0.2)[0].tolist() == [0, 1]
    assert LR.downsample(rows, len(rows), 0.2, cap=2)[0].tolist() == [0, 1]
    assert LR.downsample(rows, 0, 0.2)[0].tolist() == []


def test_ape_translation_on_a_hand_computed_case():
    from sps_amd.trajectory import ape_translation
    ref = [np.eye(4) for _ in range(4)]
    est = [np.eye(4) for _ in range(4)]
    est[0][:3, 3] = [3.0, 4.0, 0.0]                                   # 5
    est[1][:3, 3] = [0.0, 0.0, 1.0]                                   # 1
    est[2][:3, 3] = [0.0, 2.0, 0.0]                                   # 2
    est[3][:3, :3] = LR.perturbation(0, 0, 0, 30.0)[:3, :3]           # 0: rotation does not enter
    s = ape_translation(est, ref)
    assert s["rmse"] == pytest.approx(np.sqrt(30.0 / 4.0)) and s["mean"] == pytest.approx(2.0)
    assert s["median"] == pytest.approx(1.5) and s["min"] == 0.0 and s["max"] == pytest.approx(5.0)
    assert s["std"] == pytest.approx(np.sqrt(30.0 / 4.0 - 4.0))
    assert list(s) == ["rmse", "mean", "median", "std", "min", "max"]
    with pytest.raises(ValueError):
        ape_translation(est, ref[:3])


def test_write_trajectory_round_trips(tmp_path):
    from sps_amd.trajectory import read_trajectory, write_trajectory
    rng = np.random.default_rng(3)
    poses = [LR.perturbation(*rng.normal(size=3), 40.0 * k, 3.0) for k in range(5)]
    stamps = [f"{1656500000.0 + 0.5 * i:.6f}" for i in range(5)]
    path = tmp_path / "traj.txt"
    write_trajectory(path, stamps, poses)
    lines = open(path).read().splitlines()
    assert len(lines) == 5 and all(len(l.split()) == 13 for l in lines)
    got_stamps, got = read_trajectory(path)
    assert got_stamps == stamps
    np.testing.assert_array_equal(got, np.array(poses))              # the same bits


# ---- LocalisationLoop with stub stages -------------------------------------------------------------------------------------
class _StubPose:
    def __init__(self, pose, status):
        self.pose, self.status = pose, status


class _StubPendingPose:
    def __init__(self, res):
        self._res = res

    def result(self):
        return self._res


class _StubLocaliser:
    """Answers guess -> shift @ guess; ``fail_at`` frames answer status 2 with the guess itself."""
    device = "cpu"

    def __init__(self, shift, fail_at=()):
        self.shift, self.fail_at, self.calls = shift, set(fail_at), []

    def submit(self, rows, count, T_init):
        k = len(self.calls)
        self.calls.append((rows, count, np.array(T_init)))
        if k in self.fail_at:
            return _StubPendingPose(_StubPose(np.array(T_init), 2))
        return _StubPendingPose(_StubPose(self.shift @ np.array(T_init), 0))


class _StubFrame:
    def __init__(self, filtered):
        self.filtered = filtered


class _StubPending:
    def __init__(self, filtered):
        self._f = filtered

    def result(self):
        return _StubFrame(self._f)


class _StubPoseFilter:
    def __init__(self):
        self.seen = []

    def submit(self, scan, pose):
        self.seen.append(np.array(pose))
        return _StubPending(scan[:3])


class _StubCVMFilter:
    def __init__(self):
        self.added, self.submits = [], 0

    def add_pose(self, T):
        self.added.append(np.array(T))

    def submit(self, scan):
        self.submits += 1
        return _StubPending(scan[:2])


def _motion(k):
    return LR.perturbation(0.5, 0.01 * k, 0.0, 1.0)


def test_loop_guess_order_and_filter_pose():
    from sps_amd.localiser import LocalisationLoop
    from sps_amd.sps_filters import ConstantVelocityModel
    shift = LR.perturbation(0.5, 0.0, 0.0, 1.0)
    loc, f = _StubLocaliser(shift), _StubPoseFilter()
    T0 = LR.perturbation(2.0, 1.0, 0.0, 10.0)
    loop = LocalisationLoop(f, loc, T0)
    scan = np.arange(40, dtype=np.float32).reshape(10, 4)
    steps = [loop.step(scan) for _ in range(6)]
    np.testing.assert_array_equal(steps[0].guess, T0)                                  # nothing corrected yet
    for k in (1, 2, 3):
        np.testing.assert_array_equal(steps[k].guess, steps[k - 1].pose)               # the last corrected pose
    cvm = ConstantVelocityModel()
    cvm.poses = [s.pose for s in steps[:4]]
    np.testing.assert_array_equal(steps[4].guess, cvm.predict())                       # four poses: constant velocity
    assert not np.array_equal(steps[4].guess, steps[3].pose)
    for k, s in enumerate(steps):
        np.testing.assert_array_equal(f.seen[k], s.guess)                              # the filter got the guess
        np.testing.assert_array_equal(loc.calls[k][2], s.guess)                        # and so did the localiser
        np.testing.assert_array_equal(s.pose, shift @ s.guess)
        assert loc.calls[k][1] == 3 and not s.flagged
    assert len(loop.poses) == 6


def test_loop_feeds_add_pose_the_corrected_pose_and_falls_back_on_status_2():
    from sps_amd.localiser import LocalisationLoop
    shift = LR.perturbation(0.5, 0.0, 0.0, 1.0)
    loc, f = _StubLocaliser(shift, fail_at=(2,)), _StubCVMFilter()
    T0 = LR.perturbation(2.0, 1.0, 0.0, 10.0)
    loop = LocalisationLoop(f, loc, T0)
    scan = np.zeros((5, 4), dtype=np.float32)
    steps = [loop.step(scan) for _ in range(4)]
    assert f.submits == 4 and len(f.added) == 4
    for k, s in enumerate(steps):
        np.testing.assert_array_equal(f.added[k], s.pose)                              # never a replayed pose: only the loop's own
    assert [s.flagged for s in steps] == [False, False, True, False]
    np.testing.assert_array_equal(steps[2].pose, steps[2].guess)                       # status 2: the guess is handed on
    np.testing.assert_array_equal(steps[2].guess, steps[1].pose)
    np.testing.assert_array_equal(steps[3].guess, steps[2].pose)
    np.testing.assert_array_equal(steps[0].pose, shift @ T0)


# ---- the device buffers' layouts and their parsing ---------------------------------------------------------------------
def test_the_layouts_are_the_formulas_the_buffers_were_written_with():
    from sps_amd.localiser import _batch_layout, _pose_layout
    for K in (0, 1, 2, 5):
        for with_normal in (False, True):
            size = 19 + 32 * K if with_normal else 19 + 4 * K
            for pyramid in (False, True):
                for L in (None, 1, 3):
                    w = 2 if L is None else 2 * L
                    for integrate in (False, True):
                        for carve in (False, True):
                            o = _pose_layout(K, with_normal, pyramid, L, integrate, carve)
                            case = (K, with_normal, pyramid, L, integrate, carve)
                            assert (o["T_out"], o["status"], o["n_points"], o["trace"], o["normal"]) == (0, 16, 18, 19, 19 + 4 * K), case
                            assert o["size"] == o["levels"] == size, case
                            upd_at = size + ((K + 1) // 2 if pyramid else 0)
                            carve_at = upd_at + (w if integrate else 0)
                            assert (o["update"], o["carve"], o["total"]) == (upd_at, carve_at, carve_at + (w if carve else 0)), case
                            assert o["hands_on"] == (0, 16 * 8), case              # T_out and the status word, in bytes
    for K, I in ((1, 0), (1, 5), (3, 2), (64, 30)):
        for with_normal in (False, True):
            for integrate in (False, True):
                for carve in (False, True):
                    o = _batch_layout(K, I, with_normal, integrate, carve)
                    at = [0, 16 * K, 18 * K, 18 * K + 1, 18 * K + 3, 18 * K + 19, 20 * K + 19, 20 * K + 19 + 4 * K * I]
                    assert [o[k] for k in ("T_out", "status", "n_points", "best", "T_best", "final", "trace", "normal")] == at
                    size = at[-1] + (28 * K * I if with_normal else 0)
                    assert o["size"] == o["update"] == size and o["carve"] == size + (2 if integrate else 0)
                    assert o["total"] == size + (2 if integrate else 0) + (2 if carve else 0)
                    assert _batch_layout(K, I, with_normal)["total"] == size
                    assert o["hands_on"] == ((18 * K + 3) * 8, (18 * K + 1) * 8 + 4)   # T_best and best[1], in bytes


class _DoneEvent:
    def __init__(self):
        self.waits = 0

    def synchronize(self):
        self.waits += 1


def _words(h, at, values):
    """int32 ``values`` from double ``at`` of the float64 buffer h on"""
    h[at:].view(np.int32)[:len(values)] = values


@pytest.mark.parametrize("L", [None, 3])
def test_the_pending_objects_parse_buffers_filled_by_hand(L):
    import torch
    from sps_amd.localiser import (MapCarveResult, MapUpdateResult, PendingMapCarve, PendingMapUpdate, PendingPose, PendingPoses)
    n = L or 1
    upd_words, carve_words = np.arange(100, 100 + 4 * n), np.arange(200, 200 + 4 * n)
    upds = [MapUpdateResult(*(int(v) for v in upd_words[4 * l:4 * l + 4]), 77) for l in range(n)]
    carves = [MapCarveResult(*(int(v) for v in carve_words[4 * l:4 * l + 4]), 77) for l in range(n)]
    want_upd, want_carve = (upds[0], carves[0]) if L is None else (tuple(upds), tuple(carves))
    # ---- a frame: K = 5 slots of which 3 ran, normal rows, a pyramid's levels, update and carve ----
    K, w = 5, 2 * n
    h = np.zeros(19 + 32 * K + 3 + 2 * w)
    h[:16] = np.arange(16) + 0.5
    _words(h, 16, [1, 3, 60, 9])                                      # status, slots run, n_corr, (level)
    _words(h, 18, [77, 12])                                           # n_points, n_sources in the pad
    h[19:19 + 4 * K] = np.arange(4 * K) + 1000.0
    h[19 + 4 * K:19 + 32 * K] = np.arange(28 * K) + 2000.0
    _words(h, 19 + 32 * K, [0, 1, 2, -1, -1])                         # levels: (K + 1) // 2 = 3 doubles
    _words(h, 19 + 32 * K + 3, upd_words)
    _words(h, 19 + 32 * K + 3 + w, carve_words)
    ev = _DoneEvent()
    r = PendingPose(K, True, torch.from_numpy(h), ev, None, True, L, True, True).result()
    assert ev.waits == 1
    assert np.array_equal(r.pose, (np.arange(16) + 0.5).reshape(4, 4))
    assert (r.status, r.iterations, r.n_corr, r.n_points, r.n_sources) == (1, 3, 60, 77, 12)
    assert np.array_equal(r.trace, (np.arange(4 * K) + 1000.0).reshape(K, 4)[:3])
    assert np.array_equal(r.normal, (np.arange(28 * K) + 2000.0).reshape(K, 28)[:3])
    assert r.rmse == np.sqrt(1009.0 / 60) and r.levels.tolist() == [0, 1, 2]
    assert r.map_update == want_upd and r.map_carve == want_carve
    # the plain frame: no normal rows, no pyramid, no map work
    r = PendingPose(K, False, torch.from_numpy(h[:19 + 4 * K].copy()), _DoneEvent(), None).result()
    assert (r.status, r.iterations, r.n_points) == (1, 3, 77) and r.normal is None and r.levels is None
    assert r.map_update is None and r.map_carve is None and np.array_equal(r.trace, (np.arange(4 * K) + 1000.0).reshape(K, 4)[:3])
    # ---- integrate / carve: int32, n_points (+ pad) | info ----
    m = np.zeros(4 + 4 * n, dtype=np.int32)
    m[0] = 77
    m[4:] = upd_words
    assert PendingMapUpdate(torch.from_numpy(m), _DoneEvent(), None, L).result() == want_upd
    m[4:] = carve_words
    assert PendingMapCarve(torch.from_numpy(m), _DoneEvent(), None, L).result() == want_carve
    if L is not None:
        return                                                        # the batch works on the single map: four words each
    # ---- a batch of 2 hypotheses, 3 slots, behind 7 doubles of something else ----
    K, I, at = 2, 3, 7
    b = np.zeros(at + 20 * K + 19 + 32 * K * I + 4)
    v = b[at:]
    v[:16 * K] = np.arange(16 * K) + 0.25
    _words(v, 16 * K, [0, 2, 55, 0, 2, 0, 0, 0])                      # hypothesis 0: status 0 after 2 slots; 1: status 2, none run
    _words(v, 18 * K, [77])
    _words(v, 18 * K + 1, [0, 0])                                     # best, its status
    v[18 * K + 3:18 * K + 19] = np.arange(16) + 0.75
    v[18 * K + 19:20 * K + 19] = [9.5, 70.0, 1.5, 3.0]
    v[20 * K + 19:20 * K + 19 + 4 * K * I] = np.arange(4 * K * I) + 1000.0
    v[20 * K + 19 + 4 * K * I:20 * K + 19 + 32 * K * I] = np.arange(28 * K * I) + 2000.0
    _words(v, 20 * K + 19 + 32 * K * I, upd_words)
    _words(v, 20 * K + 19 + 32 * K * I + 2, carve_words)
    r = PendingPoses(K, I, True, torch.from_numpy(b), _DoneEvent(), None, at, True, True).result()
    assert r.best == 0 and np.array_equal(r.pose, (np.arange(16) + 0.75).reshape(4, 4))
    assert r.scores.tolist() == [9.5, 1.5] and r.counts.tolist() == [70, 3]
    assert r.map_update == want_upd and r.map_carve == want_carve
    a, c = r.results
    assert (a.status, a.iterations, a.n_corr, a.n_points) == (0, 2, 55, 77) and (c.status, c.iterations, c.n_corr) == (2, 0, 0)
    assert np.array_equal(a.pose, (np.arange(16) + 0.25).reshape(4, 4)) and np.array_equal(c.pose, (np.arange(16) + 16.25).reshape(4, 4))
    assert np.array_equal(a.trace, (np.arange(8) + 1000.0).reshape(2, 4)) and c.trace.shape == (0, 4) and np.isnan(c.rmse)
    assert np.array_equal(a.normal, (np.arange(56) + 2000.0).reshape(2, 28)) and a.rmse == np.sqrt(1005.0 / 55)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------
def test_localiser_symbols_are_declared_and_exported():
    from sps_amd import _native
    hdr = open(os.path.join(ROOT, "include", "sps_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("sps_loc_downsample", "sps_loc_align", "sps_loc_downsample_scratch", "sps_loc_align_scratch"):
        assert re.search(r"\b%s\s*\(" % name, hdr), f"include/sps_hip.h does not declare {name}"
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
    assert _native.lib.sps_version() == 202
    assert _native.lib.sps_loc_downsample_scratch(1000) >= 2048 * 12
    assert _native.lib.sps_loc_align_scratch(64) >= 2 * 29 * 8 + 4
    assert _native.lib.sps_loc_align_scratch(-1) < 0
    # bad arguments are rejected before any device call
    assert _native.lib.sps_loc_align(None, None, None, 0, None, 1, 1, 0.0, 0.0, None, None, None, None, None, None) < 0
    assert _native.lib.sps_loc_downsample(None, None, 3, 0, None, 0.2, None, 0, None, None, None) < 0
