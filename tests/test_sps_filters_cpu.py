"""Host-side tests of the node-complete SPS filters (sps_amd/sps_filters.py, sps_amd/replay.py): the constant-velocity
model against matrices captured from the reference node (tools/capture_sps_node_goldens.py), the sequence replay, the
metric derivation, the log format and the declaration of sps_filter_finish.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests.sps_node_reference import finish_reference, sums_from_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_constant_velocity_model_reproduces_the_reference_node():
    """Every matrix of cvm_poses.npz within 1e-12 of the largest element (the inverse of a rigid transform is well
    conditioned; LAPACK builds may differ in the last bits).  Lengths 1 and 3 give the identity, 4 and 10 use three
    relative motions, 11 and 25 nine."""
    from sps_amd.sps_filters import ConstantVelocityModel
    z = np.load(os.path.join(GOLD, "cvm_poses.npz"))
    assert z["lengths"].tolist() == [1, 3, 4, 10, 11, 25]
    for n in z["lengths"].tolist():
        poses, want = z[f"poses_{n}"], z[f"pred_{n}"]
        assert len(poses) == n and np.array_equal(poses[0], np.eye(4))
        cvm = ConstantVelocityModel()
        for T in poses[1:]:                                  # the list starts as [I]
            cvm.add_pose(T)
        assert len(cvm.poses) == n
        before = [p.copy() for p in cvm.poses]
        got = cvm.predict()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), n
        if n < 4:
            assert np.array_equal(got, np.eye(4))
        else:
            assert not np.allclose(got, poses[-1])
        for a, b in zip(cvm.poses, before):                  # predicting leaves the list alone
            assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        ConstantVelocityModel().add_pose(np.eye(3))


def test_constant_velocity_model_keeps_the_oldest_rotation_and_the_mean_column():
    """The details the issue names, on a list where they are visible: nine motions past ten poses, the rotation of the
    OLDEST of them, the whole fourth column from the mean."""
    from sps_amd.sps_filters import ConstantVelocityModel
    z = np.load(os.path.join(GOLD, "cvm_poses.npz"))
    poses = list(z["poses_25"])
    cvm = ConstantVelocityModel()
    for T in poses[1:]:
        cvm.add_pose(T)
    rel = [np.linalg.inv(poses[25 - i]) @ poses[25 - i + 1] for i in range(2, 11)]
    want = rel[-1].copy()
    want[:, 3] = np.mean(rel, axis=0)[:, 3]
    np.testing.assert_allclose(cvm.predict(), poses[-1] @ want, rtol=0, atol=1e-12 * np.abs(poses[-1]).max())
    newest = rel[0].copy()
    newest[:, 3] = np.mean(rel, axis=0)[:, 3]
    assert np.abs(cvm.predict() - poses[-1] @ newest).max() > 1e-6


def _tree(root, stems, n_poses=None):
    seq = os.path.join(root, "sequence", "7")
    os.makedirs(os.path.join(seq, "scans"))
    os.makedirs(os.path.join(seq, "poses"))
    np.savetxt(os.path.join(seq, "map_transform"), 2.0 * np.eye(4), delimiter=",")
    for k, s in enumerate(stems):
        np.save(os.path.join(seq, "scans", s + ".npy"), np.full((3, 4), float(k)))
    for k, s in enumerate(stems[:n_poses]):
        T = np.eye(4)
        T[0, 3] = k
        np.savetxt(os.path.join(seq, "poses", s + ".txt"), T, delimiter=",")


def test_scan_replay_orders_by_stamp_value_and_checks_the_counts(tmp_path):
    from sps_amd.replay import ScanReplay
    stems = ["10.5", "9.5", "100.25", "9.75"]                          # unequal lengths: a string sort would misorder
    _tree(str(tmp_path / "a"), stems)
    got = list(ScanReplay(str(tmp_path / "a"), 7))
    assert [g[0] for g in got] == ["9.5", "9.75", "10.5", "100.25"]
    assert sorted(s + ".npy" for s in stems) != [g[0] + ".npy" for g in got]
    for stamp, scan, pose, map_tr in got:
        k = stems.index(stamp)
        assert scan.shape == (3, 4) and (scan == k).all() and pose[0, 3] == k and pose.shape == (4, 4)
        np.testing.assert_array_equal(map_tr, 2.0 * np.eye(4))
    eq = [f"16565000{k:02d}.500000" for k in (3, 1, 2)]                # equal lengths: the reference's order
    _tree(str(tmp_path / "b"), eq)
    rp = ScanReplay(str(tmp_path / "b"), "7")
    assert len(rp) == 3 and rp.scans == sorted(os.listdir(rp.scans_pth)) and rp.poses == sorted(os.listdir(rp.poses_pth))
    _tree(str(tmp_path / "c"), eq, n_poses=2)
    with pytest.raises(AssertionError, match="Must have the same length!!"):
        ScanReplay(str(tmp_path / "c"), 7)


def test_synthetic_tree_replays_into_the_map_frame(tmp_path):
    from sps_amd.replay import ScanReplay, write_synthetic_tree
    from sps_amd import synthetic
    from sps_amd.datasets import util
    pc_map = write_synthetic_tree(str(tmp_path), 3, n_azimuth=60, n_beams=8)
    assert np.array_equal(np.load(tmp_path / "maps" / "base_map.asc.npy"), pc_map)
    frames = list(ScanReplay(str(tmp_path), "synthetic"))
    assert len(frames) == 3
    for i, (stamp, scan, pose, map_tr) in enumerate(frames):
        world = synthetic.lidar_scan(100 + i, x_offset=0.5 * i, n_azimuth=60, n_beams=8)
        assert scan.dtype == np.float32 and scan.shape == world.shape
        back = util.transform_point_cloud(scan[:, :3].astype(np.float64), map_tr @ pose)
        np.testing.assert_allclose(back, world[:, :3], atol=1e-4)
        np.testing.assert_array_equal(scan[:, 3], world[:, 3])


def test_metrics_from_a_sums_row_equal_the_reference_golden():
    from sps_amd.sps_filters import node_metrics
    z = np.load(os.path.join(GOLD, "calculate_metrics.npz"))
    assert int(z["n"]) >= 7
    for i in range(int(z["n"])):
        with np.errstate(all="ignore"):
            m = node_metrics(sums_from_labels(z[f"gt{i}"], z[f"pred{i}"]))
        got = np.array([m["precision"], m["recall"], m["f1"], m["accuracy"], m["dIoU"]], dtype=np.float64)
        np.testing.assert_array_equal(got, z[f"out{i}"])                  # NaN == NaN here
    # loss and R2 from the regression sums (nn.MSELoss, torchmetrics R2Score)
    rng = np.random.default_rng(5)
    s, g = rng.uniform(size=500).astype(np.float32), rng.uniform(size=500).astype(np.float32)
    ref = finish_reference(s, np.c_[np.zeros((500, 3), np.float32), g], np.zeros((500, 5), np.float32), 0, 0.84, False)
    m = node_metrics(ref["sums"])
    s64, g64 = s.astype(np.float64), g.astype(np.float64)
    np.testing.assert_allclose(m["loss"], np.mean((s64 - g64) ** 2), rtol=1e-12)
    np.testing.assert_allclose(m["r2"], 1 - np.sum((s64 - g64) ** 2) / np.sum((g64 - g64.mean()) ** 2), rtol=1e-9)
    assert m["count"] == 500 and m["tp"] + m["fp"] + m["fn"] + m["tn"] == 500


def test_log_lines_have_the_nodes_format():
    from sps_amd.sps_filters import SPSResult
    res = SPSResult(filtered=torch.zeros(1234, 4), scores=torch.zeros(5000), labels=torch.zeros(5000, dtype=torch.int32),
                    cloud_tr=torch.zeros(5000, 4), submap=torch.zeros(777, 4), n_scan_voxels=4321, n_submap_voxels=777,
                    loss=0.12345, r2=-0.5, dIoU=0.25, accuracy=0.875, precision=0.3333333, recall=1.0, f1=0.5,
                    counts=None, pose=None, t_total=0.025, t_prune=0.002, t_infer=0.0, t_finish=0.001)
    metrics, timing = res.log_lines()
    assert metrics == "dIoU: 0.250 accuracy: 0.875 precision: 0.333 recall: 1.000 f1: 0.500 "
    assert timing == ("T: 0.025 [40.00 Hz] P: 0.002 [500.00 Hz] I: 0.000 [0.00 Hz] L: 0.123 r2: -0.500 "
                      "N: 5000 n: 1234 S: 4321 M: 777 ")
    res.loss = res.r2 = res.dIoU = res.accuracy = res.precision = res.recall = res.f1 = None     # a scan without labels
    metrics, timing = res.log_lines()
    assert metrics == "dIoU: nan accuracy: nan precision: nan recall: nan f1: nan " and "L: nan r2: nan " in timing


def test_header_declares_sps_filter_finish_and_the_binding_lists_it():
    hdr = open(os.path.join(ROOT, "include", "sps_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+sps_filter_finish\s*\(([^;]*)\)\s*;", code)
    assert m, "include/sps_hip.h does not declare sps_filter_finish"
    args = m.group(1)
    for name in ("scores_dev", "raw_dev", "label_col", "batch_dev", "counts_dev", "eps", "keep_strict", "filtered_dev",
                 "count_dev", "labels_dev", "cloud_tr_dev", "submap_dev", "sums_dev", "stream"):
        assert re.search(rf"\b{name}\b", args), name
    from sps_amd import _native
    assert "sps_filter_finish" in _native.EXPORTS and hasattr(_native.lib, "sps_filter_finish")
    assert _native.lib.sps_version() == _native.ABI_VERSION == 202       # additive: the ABI version does not change
    # argument checks fail before any device work
    assert _native.lib.sps_filter_finish(None, None, 0, None, 4, 4, 3, None, None, 0.84, 0, None, None, None, None, None,
                                         None, None) != 0
