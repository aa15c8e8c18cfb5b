"""GPU tests of the node-complete SPS filters (sps_amd/sps_filters.py), the native call under them (sps_filter_finish,
include/sps_hip.h) and the sequence driver (scripts/filter_sequence.py), against the numpy restatement of the nodes in
tests/sps_node_reference.py and against pipeline.StableFilter."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from sps_amd._native import SpsError
from sps_amd.datasets import util
from tests.helpers import CFG, net_from_params, straddle_params
from tests.sps_node_reference import finish_reference

pytestmark = pytest.mark.gpu

VS = CFG["MODEL"]["VOXEL_SIZE"]
EPS = CFG["FILTER"]["THRESHOLD"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def net():
    params = straddle_params(O.random_params(seed=0), synthetic.small_scene(seed=11, n_scan=2500))
    return net_from_params(params).cuda().eval().freeze()


@pytest.fixture(scope="module")
def map_pts():
    return synthetic.build_map(n_azimuth=400, n_beams=32)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ctx():
    from sps_amd.models.models import get_context
    return get_context(0, stream())


def _pose(k):
    a = 0.1 + 0.15 * k
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = [0.8 * k, -0.3 * k, 0.05 * k]
    return T


def _sensor_scan(seed, T, dtype=np.float32, x_offset=0.0):
    """(x, y, z, label) rows in the sensor frame of pose T, labels with values at and around the threshold."""
    world = synthetic.lidar_scan(seed, x_offset=x_offset, n_azimuth=400, n_beams=32)
    xyz = util.inverse_transform_point_cloud(world[:, :3].astype(np.float64), T)
    lab = world[:, 3].copy()
    e = np.float32(EPS)
    lab[::7] = e
    lab[1::7] = np.nextafter(e, np.float32(0))
    return np.c_[xyz, lab].astype(dtype)


# ---- sps_filter_finish ---------------------------------------------------------------------------------------------------
def _finish(scores, raw, ld, cols, label_col, batch, n_sub, strict, outputs=True):
    n = len(scores)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ds, dr, db = d(scores), d(raw), d(batch)
    counts = torch.tensor([n_sub, 99, n + n_sub, -5, -7], dtype=torch.int32, device="cuda")
    m = max(n, 1)
    filtered = torch.full((m, cols), -1.0, device="cuda")
    labels = torch.full((m,), -1, dtype=torch.int32, device="cuda")
    cloud_tr = torch.full((m, 4), -1.0, device="cuda")
    submap = torch.full((m, 4), -1.0, device="cuda")
    sums = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    p = (lambda t: t.data_ptr()) if outputs else (lambda t: None)
    ctx().filter_finish(ds.data_ptr() if n else None, n, dr.data_ptr() if n else None, ld, cols, label_col,
                        db.data_ptr() if n else None, counts.data_ptr(), EPS, strict, p(filtered), counts.data_ptr() + 12 if outputs else None,
                        p(labels), p(cloud_tr), p(submap), p(sums), stream())
    torch.cuda.synchronize()
    return dict(filtered=filtered.cpu().numpy(), kept=int(counts[3]), labels=labels.cpu().numpy(), cloud_tr=cloud_tr.cpu().numpy(),
                submap=submap.cpu().numpy(), sums=sums.cpu().numpy(), guard=counts.cpu().numpy()[[0, 1, 2, 4]])


def _case(kind, n, rng):
    e = np.float32(EPS)
    s = rng.uniform(0, 1, n).astype(np.float32)
    raw = rng.normal(size=(n, 6)).astype(np.float32)                    # 5 columns per row, row stride 6
    raw[:, 3] = rng.uniform(0, 1, n)
    raw[::5, 3] = e
    raw[1::5, 3] = np.nextafter(e, np.float32(0))
    raw[2::5, 3] = np.nextafter(e, np.float32(1))
    if kind in ("edges", "finite"):
        s[::11] = e                                                     # kept by `<=`, dropped by `<`
        s[1::11] = np.nextafter(e, np.float32(1))
        s[2::11] = np.nextafter(e, np.float32(0))
    if kind == "edges":
        s[5::97] = np.nan
        raw[3::89, 3] = np.nan
    if kind == "all":
        s[:] = rng.uniform(0, 0.5, n)
    if kind == "none":
        s[:] = rng.uniform(0.9, 1.0, n)
    batch = rng.normal(size=(2 * max(n, 1), 5)).astype(np.float32)
    return s, raw, batch


@pytest.mark.parametrize("kind,n", [("edges", 70_001), ("finite", 70_001), ("all", 3000), ("none", 1025), ("edges", 63),
                                    ("empty", 0)])
def test_filter_finish_matches_the_numpy_restatement(kind, n):
    rng = np.random.default_rng(3)
    s, raw, batch = _case(kind, n, rng)
    n_sub = (2 * n) // 3
    got = {}
    for strict in (False, True):
        ref = finish_reference(s, raw[:, :5], batch, n_sub, EPS, strict)
        g = got[strict] = _finish(s, raw, 6, 5, 3, batch, n_sub, strict)
        k = len(ref["filtered"])
        assert g["kept"] == k
        np.testing.assert_array_equal(g["filtered"][:k], ref["filtered"])              # whole rows, input order (NaN == NaN)
        assert (g["filtered"][k:] == -1).all() and g["guard"].tolist() == [n_sub, 99, n + n_sub, -7]
        np.testing.assert_array_equal(g["labels"][:n], ref["labels"])
        np.testing.assert_array_equal(g["cloud_tr"][:n], ref["cloud_tr"])
        np.testing.assert_array_equal(g["submap"][:n_sub], ref["submap"])
        assert (g["labels"][n:] == -1).all() and (g["cloud_tr"][n:] == -1).all() and (g["submap"][n_sub:] == -1).all()
        np.testing.assert_array_equal(g["sums"][:5], ref["sums"][:5])                 # the five integer counts: exact
        np.testing.assert_allclose(g["sums"][5:], ref["sums"][5:], rtol=1e-12)        # numpy's f64 sums of the same f32 inputs
        again = _finish(s, raw, 6, 5, 3, batch, n_sub, strict)
        np.testing.assert_array_equal(again["sums"], g["sums"])                       # fixed-order sums: the same bits
        if kind == "finite":
            assert np.isfinite(g["sums"]).all() and (g["sums"][1:5] > 0).all()
        if kind == "edges" and n > 1000:
            assert np.isnan(g["sums"][5:]).all() and np.isnan(ref["sums"][5:]).all()   # NaN scores / labels reach the sums
        if kind == "all":
            assert k == n
        if kind == "none":
            assert k == 0
    if kind in ("edges", "finite"):                                                    # the two rules differ on the eps rows
        ties = int((s == np.float32(EPS)).sum())
        assert ties > 0 and got[False]["kept"] - got[True]["kept"] == ties
        np.testing.assert_array_equal(got[False]["labels"], got[True]["labels"])
    # no label column: the sums row is left alone; no outputs at all is legal
    g = _finish(s, raw, 6, 3, -1, batch, n_sub, False)
    assert (g["sums"] == -1).all() and g["kept"] == len(finish_reference(s, raw[:, :3], batch, n_sub, EPS, False)["filtered"])
    _finish(s, raw, 6, 5, 3, batch, n_sub, False, outputs=False)


# ---- SPSFilter -----------------------------------------------------------------------------------------------------------
def _check_against_reference(res, scan32, strict, eps=EPS):
    n = len(scan32)
    scores = res.scores.cpu().numpy()
    batch = np.zeros((n + res.n_submap_voxels, 5), np.float32)
    batch[:n, 1:4] = res.cloud_tr[:, :3].cpu().numpy()
    batch[n:, 1:4] = res.submap[:, :3].cpu().numpy()
    ref = finish_reference(scores, scan32, batch, res.n_submap_voxels, eps, strict)
    np.testing.assert_array_equal(res.filtered.cpu().numpy(), ref["filtered"])
    np.testing.assert_array_equal(res.labels.cpu().numpy(), ref["labels"])
    np.testing.assert_array_equal(res.cloud_tr[:, 3].cpu().numpy(), ref["labels"].astype(np.float32))
    assert (res.submap[:, 3] == 1).all() and res.submap.shape == (res.n_submap_voxels, 4)
    if scan32.shape[1] > 3:
        from sps_amd.sps_filters import node_metrics
        c = res.counts
        assert [c["count"], c["tp"], c["fp"], c["fn"], c["tn"]] == ref["sums"][:5].tolist()
        m = node_metrics(ref["sums"])
        for k in ("loss", "r2", "dIoU", "accuracy", "precision", "recall", "f1"):
            np.testing.assert_allclose(getattr(res, k), m[k], rtol=1e-9, err_msg=k)
        with np.errstate(invalid="ignore"):
            want = util.calculate_metrics(np.where(scan32[:, 3] < np.float32(eps), 0, 1), ref["labels"])
        np.testing.assert_allclose([res.precision, res.recall, res.f1, res.accuracy, res.dIoU], want, rtol=1e-12)
        s64, g64 = scores.astype(np.float64), scan32[:, 3].astype(np.float64)
        np.testing.assert_allclose(res.loss, np.mean((s64 - g64) ** 2), rtol=1e-9)
    else:
        assert res.loss is None and res.dIoU is None and res.counts is None
    return ref


@pytest.mark.parametrize("dtype,cols", [(np.float32, 4), (np.float64, 4), (np.float32, 3), (np.float32, 6)])
def test_sps_filter_equals_stable_filter_and_the_node(net, map_pts, dtype, cols):
    """scores, S, M and the three-column projection of the kept rows are bit-identical to StableFilter on the same scan and
    pose; labels, clouds, metrics and the whole kept rows equal the numpy restatement applied to those scores."""
    from sps_amd.pipeline import StableFilter
    from sps_amd.sps_filters import SPSFilter
    T = _pose(1)
    scan = _sensor_scan(77, T, dtype, x_offset=1.0)
    if cols == 3:
        scan = np.ascontiguousarray(scan[:, :3])
    if cols == 6:
        scan = np.c_[scan, np.arange(len(scan), dtype=dtype), -np.ones(len(scan), dtype)]
    f = SPSFilter(net, torch.from_numpy(map_pts), voxel_size=VS, epsilon=EPS)
    res = f(scan, T)
    want = StableFilter(net, torch.from_numpy(map_pts), voxel_size=VS, epsilon=EPS)(scan, T)
    assert torch.equal(res.scores, want.scores)
    assert (res.n_scan_voxels, res.n_submap_voxels) == (want.n_scan_voxels, want.n_submap_voxels) and want.n_submap_voxels > 0
    assert torch.equal(res.filtered[:, :3], want.filtered) and res.filtered.shape[1] == cols
    assert 0 < len(res.filtered) < len(scan)
    scan32 = scan.astype(np.float32)
    _check_against_reference(res, scan32, strict=False)
    np.testing.assert_array_equal(res.cloud_tr[:, :3].cpu().numpy(),
                                  util.transform_point_cloud(scan[:, :3].astype(np.float64), T).astype(np.float32))
    sub, _ = O.prune(O.to_coords(map_pts[:, :3], VS), O.to_coords(res.cloud_tr[:, :3].cpu().numpy(), VS), VS)
    np.testing.assert_array_equal(np.unique(res.submap[:, :3].cpu().numpy(), axis=0), np.unique(sub, axis=0))
    metrics, timing = res.log_lines()
    assert timing.endswith(f"N: {len(scan):d} n: {len(res.filtered):d} S: {res.n_scan_voxels:d} M: {res.n_submap_voxels:d} ")
    assert res.t_total > 0 and res.t_prune > 0 and res.t_infer > 0 and res.t_finish > 0
    empty = f(np.zeros((0, cols), dtype), T)
    assert empty.filtered.shape == (0, cols) and empty.scores.shape == (0,) and empty.submap.shape == (0, 4)
    assert empty.n_submap_voxels == 0 and (cols == 3 or empty.counts["count"] == 0)


def test_sps_cvm_filter_predicts_the_pose_prunes_at_02_and_keeps_strictly(net, map_pts):
    """Prune size 0.2 with the network at 0.1: scores bit-identical to StableFilter(voxel_size=0.2) -- whose forward runs
    at the network's own voxel size -- given the predicted pose explicitly; the kept set is score < eps."""
    from sps_amd.pipeline import StableFilter
    from sps_amd.sps_filters import ConstantVelocityModel, SPSCVMFilter
    f = SPSCVMFilter(net, torch.from_numpy(map_pts), voxel_size=VS, epsilon=EPS)
    assert f.prune_ds == 0.2 and f.ds == VS and f.keep_strict
    cvm = ConstantVelocityModel()
    with pytest.raises(ValueError):
        f.submit(np.zeros((4, 4), np.float32), np.eye(4))
    for k in range(6):
        T_pred = cvm.predict()
        assert np.array_equal(T_pred, np.eye(4)) == (k < 3)              # [I] + k poses: identity below four entries
        scan = _sensor_scan(90 + k, _pose(k), x_offset=0.3 * k)
        res = f(scan)
        np.testing.assert_array_equal(res.pose, T_pred)
        want = StableFilter(net, torch.from_numpy(map_pts), voxel_size=0.2, epsilon=EPS)(scan, T_pred)
        assert torch.equal(res.scores, want.scores)
        assert (res.n_scan_voxels, res.n_submap_voxels) == (want.n_scan_voxels, want.n_submap_voxels)
        _check_against_reference(res, scan, strict=True)
        s = res.scores.cpu().numpy()
        np.testing.assert_array_equal(res.filtered.cpu().numpy(), scan[s < np.float32(EPS)])
        f.add_pose(_pose(k))
        cvm.add_pose(_pose(k))
    # a score exactly eps: kept by sps_node.py's rule, dropped by this node's -- on the filters themselves
    from sps_amd.sps_filters import SPSFilter
    s0 = float(res.scores[0])
    loose = SPSFilter(net, torch.from_numpy(map_pts), voxel_size=VS, epsilon=s0, prune_voxel_size=0.2)(scan, res.pose)
    strict = SPSCVMFilter(net, torch.from_numpy(map_pts), voxel_size=VS, epsilon=s0)
    for T in cvm.poses[1:-1]:                                            # the poses the last frame was predicted from
        strict.add_pose(T)
    tight = strict(scan)
    np.testing.assert_array_equal(tight.pose, res.pose)
    assert torch.equal(loose.scores, tight.scores) and float(loose.scores[0]) == np.float32(s0)
    ties = int((loose.scores == loose.scores[0]).sum())
    assert len(loose.filtered) - len(tight.filtered) == ties >= 1


def _arrays(res):
    return {k: v.cpu().numpy().copy() for k, v in vars(res).items() if isinstance(v, torch.Tensor)}


def test_frames_in_flight_one_synchronisation_and_errors(net, map_pts, monkeypatch):
    """Three frames submitted before any result(): equal to the one-at-a-time results; submit() never synchronises and
    result() does so once; a far-out coordinate raises from result() and the next frame is clean."""
    from sps_amd.sps_filters import SPSFilter
    poses = [_pose(k) for k in range(3)]
    scans = [_sensor_scan(600 + k, poses[k], x_offset=0.5 * k) for k in range(3)]
    sync = SPSFilter(net, torch.from_numpy(map_pts), voxel_size=VS, epsilon=EPS)
    want = [sync(s, T) for s, T in zip(scans, poses)]
    want_a = [_arrays(w) for w in want]
    f = SPSFilter(net, torch.from_numpy(map_pts), voxel_size=VS, epsilon=EPS)
    f(scans[0], poses[0])                                                # (the arena is sized by the first frame)
    calls = []
    real_stream_sync, real_sync = torch.cuda.Stream.synchronize, torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (calls.append("stream"), real_stream_sync(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("device"), real_sync(*a, **k))[1])
    for name in ("item", "cpu", "tolist", "numpy"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda real, name: lambda self, *a, **k: (
            calls.append(name) if self.is_cuda else None, real(self, *a, **k))[1])(real, name))
    pend = [f.submit(s, T) for s, T in zip(scans, poses)]
    assert calls == []                                                   # nothing synchronised while issuing three frames
    got = [p.result() for p in pend]
    assert calls == ["stream"] * 3                                       # result() is the only synchronisation
    monkeypatch.undo()
    for _ in range(2):
        f(scans[2], poses[2])                                            # later frames reuse nothing of earlier ones
    for g, w, wa in zip(got, want, want_a):
        a = _arrays(g)
        assert a.keys() == wa.keys() and len(a) == 5
        for k in wa:
            np.testing.assert_array_equal(a[k], wa[k], err_msg=k)
        assert (g.n_scan_voxels, g.n_submap_voxels, g.counts) == (w.n_scan_voxels, w.n_submap_voxels, w.counts)
        assert (g.loss, g.r2, g.dIoU, g.f1) == (w.loss, w.r2, w.dIoU, w.f1)      # fixed-order sums: the same bits
    bad = scans[1].copy()
    bad[0, 0] = 3.0e4
    with pytest.raises(SpsError):
        f(bad, poses[1])
    after = _arrays(f(scans[0], poses[0]))
    for k, v in after.items():
        np.testing.assert_array_equal(v, want_a[0][k], err_msg=k)


# ---- scripts/filter_sequence.py ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sps", "sps_cvm", "raw", "mask"])
def test_filter_sequence_cli_prints_a_line_pair_per_frame(name, tmp_path):
    out = tmp_path / "clouds"
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "scripts", "filter_sequence.py"), "--filter", name,
           "--synthetic", "6", "--out", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("[")]
    assert len(lines) == 12                                              # one line pair per frame
    stamps = [l[1:l.index("]")] for l in lines]
    assert stamps[0::2] == stamps[1::2] and [float(s) for s in stamps[0::2]] == sorted(float(s) for s in stamps[0::2])
    assert "sequence means over 6 frames" in r.stdout
    files = sorted(os.listdir(out))
    assert files == [s + ".npy" for s in stamps[0::2]]
    if name != "mask":
        assert all(" dIoU: " in " " + l for l in lines[0::2]) and all("T: " in l and " N: " in l and " M: " in l for l in lines[1::2])
        kept = [np.load(out / f_) for f_ in files]
        assert all(k.shape[1] == 4 for k in kept)
        n_in = [int(l.split(" N: ")[1].split()[0]) for l in lines[1::2]]
        if name == "raw":
            assert [len(k) for k in kept] == n_in                        # epsilon = 2: every point passes
