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
