"""GPU tests of the online 4DMOS / MapMOS / mask filters (sps_amd/baseline_filters.py) and the native pieces under them
(include/sps_hip.h, "online baseline filters"): the device-count head forward, the row writer, the radius crop, the label
filter and the device-count transform, against the eager model calls and the reference's numpy steps."""
import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from sps_amd._native import ERR_ITEMCAP, SpsError
from sps_amd.datasets import util
from tests.baseline_reference import crop_golden, crop_indices, mos4d_window_rows
from tests.helpers import state_dict_from_params

pytestmark = pytest.mark.gpu


def stream():
    return torch.cuda.current_stream().cuda_stream


def ctx():
    from sps_amd.models.models import get_context
    return get_context(0, stream())


@pytest.fixture(scope="module")
def mos4d():
    from sps_amd.models.baselines import MOS4DNet
    p = O.random_params(seed=4, out_channels=3)
    m = MOS4DNet(0.2)
    m.MinkUNet.load_state_dict(state_dict_from_params(p, prefix=""))
    return p, m.cuda().eval().freeze()


@pytest.fixture(scope="module")
def mapmos():
    from sps_amd.models.baselines import MapMOSNet
    p = O.random_params(seed=6, out_channels=1)
    m = MapMOSNet(0.1)
    m.MinkUNet.load_state_dict(state_dict_from_params(p, prefix=""))
    return p, m.cuda().eval().freeze()


def _pose(k):
    a = 0.15 * k
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = [0.8 * k, -0.3 * k, 0.05 * k]
    return T


def _scan(seed, n_az=150, dtype=np.float32):
    return synthetic.lidar_scan(seed=seed, n_beams=32, n_azimuth=n_az).astype(dtype)     # (x, y, z, s), sensor frame


def _rows(pts, t):
    return np.concatenate([np.zeros((len(pts), 1), np.float32), pts.astype(np.float32),
                           np.full((len(pts), 1), t, np.float32)], 1)


# ---- native pieces -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["mos4d", "mapmos"])
def test_forward_head_n_equals_forward_head(which, mos4d, mapmos):
    """sps_forward_head_n == sps_forward_head bit for bit (3 channels without features, 1 channel with per-point
    features), n_max > *n_dev, rows past *n_dev untouched, *n_dev == 0 followed by a normal forward."""
    p, m = mos4d if which == "mos4d" else mapmos
    oc, vs = (3, 0.2) if which == "mos4d" else (1, 0.1)
    a, b = _scan(41)[:, :3], _scan(42)[:, :3] + np.float32(0.5)
    rows = np.concatenate([_rows(a, 0), _rows(b, -1 if which == "mapmos" else 1)])
    n = len(rows)
    feats = np.concatenate([np.ones(len(a), np.float32), np.full(len(b), 2.0, np.float32)]) if which == "mapmos" else None
    pad = 1000
    dev = torch.full((n + pad, 5), 7.5e8, dtype=torch.float32, device="cuda")    # padding rows would be a range error
    dev[:n] = torch.from_numpy(rows).cuda()
    fdev = None if feats is None else torch.full((n + pad,), 1e6, device="cuda")
    if fdev is not None:
        fdev[:n] = torch.from_numpy(feats).cuda()
    m._sync_weights(ctx())
    want = torch.full((n, oc + 1), -7.0, device="cuda")
    ctx().forward_head(dev.data_ptr(), 5, n, vs, None if fdev is None else fdev.data_ptr(), 0.0, want.data_ptr(), oc + 1, 0,
                       stream())
    for count in (n, n - 333, 0, n):
        cnt = torch.tensor([5, count], dtype=torch.int32, device="cuda")
        out = torch.full((n + pad, oc + 1), -7.0, device="cuda")
        ctx().forward_head_n(dev.data_ptr(), 5, n + pad, cnt.data_ptr() + 4, vs, None if fdev is None else fdev.data_ptr(),
                             0.0, out.data_ptr(), oc + 1, 0, stream())
        ctx().check_errors(stream())
        assert (out[count:] == -7.0).all() and (out[:, oc] == -7.0).all()
        if count == n:
            assert torch.equal(out[:n], want)
        elif count:
            ref = torch.full((count, oc + 1), -7.0, device="cuda")
            ctx().forward_head(dev.data_ptr(), 5, count, vs, None if fdev is None else fdev.data_ptr(), 0.0, ref.data_ptr(),
                               oc + 1, 0, stream())
            assert torch.equal(out[:count], ref)
    got = want[:, 2].cpu().numpy() if which == "mos4d" else want[:, 0].cpu().numpy()
    ref, _ = O.head_forward(p, rows, vs, features=None if feats is None else O.mapmos_features(
        np.concatenate([np.ones(len(a)), np.zeros(len(b))])))
    np.testing.assert_allclose(got, ref[:, 2 if which == "mos4d" else 0], rtol=0, atol=2e-4)


def test_radius_crop_matches_reference_golden(mapmos):
    """sps_radius_crop: the reference node's selected indices exactly (float64 and float32 maps, points on the sphere and
    1 ulp off it), ascending map order, rows (0, x, y, z, -1), features, counts; capacity overflow -> SPS_ERR_ITEMCAP."""
    maps, poses, r = crop_golden()
    for tag, (mp, sels) in maps.items():
        dmap = torch.from_numpy(np.ascontiguousarray(mp)).cuda()
        scratch = torch.empty(max(1, -(-len(mp) // 1024)), dtype=torch.int32, device="cuda")
        for T, sel in zip(poses, sels):
            n_scan = 7
            rows = torch.full((n_scan + len(mp), 5), 99.0, device="cuda")
            feats = torch.full((n_scan + len(mp),), 99.0, device="cuda")
            counts = torch.zeros(2, dtype=torch.int32, device="cuda")
            ctx().radius_crop(dmap.data_ptr(), tag == "64", 3, len(mp), T, r, scratch.data_ptr(), n_scan, rows.data_ptr(), 5,
                              len(mp), feats.data_ptr(), 2.0, counts.data_ptr(), stream())
            ctx().check_errors(stream())
            k = len(sel)
            assert counts.tolist() == [k, n_scan + k]
            want = np.zeros((k, 5), np.float32)
            want[:, 1:4] = mp[sel].astype(np.float32)
            want[:, 4] = -1
            np.testing.assert_array_equal(rows[n_scan:n_scan + k].cpu().numpy(), want)
            assert (rows[:n_scan] == 99).all() and (rows[n_scan + k:] == 99).all()
            assert (feats[n_scan:n_scan + k] == 2).all() and (feats[:n_scan] == 99).all()
            np.testing.assert_array_equal(crop_indices(mp, T[:3, 3], r), sel)
        # capacity overflow: clamped, reported once, the next call is clean
        T, sel = poses[0], sels[0]
        ctx().radius_crop(dmap.data_ptr(), tag == "64", 3, len(mp), T, r, scratch.data_ptr(), 0, rows.data_ptr(), 5, 10,
                          None, 0.0, counts.data_ptr(), stream())
        with pytest.raises(SpsError) as ei:
            ctx().check_errors(stream())
        assert ei.value.code == ERR_ITEMCAP and counts.tolist() == [10, 10]
        ctx().check_errors(stream())


def test_label_filter_labels_compaction_and_counts():
    rng = np.random.default_rng(2)
    n = 5000
    logits = rng.normal(size=(n, 3)).astype(np.float32)
    logits[::17, 2] = 0.0
    logits[3::101, 2] = np.nan
    rows = rng.normal(size=(n, 4)).astype(np.float32)
    rows[::9, 3] = np.float32(0.84)
    lab = torch.empty(n, device="cuda")
    out = torch.full((n, 4), -1.0, device="cuda")
    counts = torch.zeros(5, dtype=torch.int32, device="cuda")
    dl, dr = torch.from_numpy(logits).cuda(), torch.from_numpy(rows).cuda()
    ctx().label_filter(dl.data_ptr() + 8, 3, n, dr.data_ptr(), 4, dr.data_ptr() + 12, 4, lab.data_ptr(), out.data_ptr(),
                       counts.data_ptr(), stream())
    pred = (logits[:, 2] > 0).astype(np.int64)
    np.testing.assert_array_equal(lab.cpu().numpy(), pred.astype(np.float32))
    keep = pred == 0
    c = counts.tolist()
    assert c[0] == keep.sum()
    np.testing.assert_array_equal(out[:c[0]].cpu().numpy(), np.c_[rows[keep, :3], np.zeros(keep.sum(), np.float32)])
    gt = np.where(rows[:, 3] < np.float32(0.84), 0, 1)
    assert c[1:] == [int(((gt == 1) & (pred == 1)).sum()), int(((gt == 0) & (pred == 1)).sum()),
                     int(((gt == 1) & (pred == 0)).sum()), int(((gt == 0) & (pred == 0)).sum())]


# ---- 4DMOS -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_index,dtype", [(0, np.float32), (1234, np.float64)])
def test_mos4d_filter_matches_node_loop(mos4d, first_index, dtype):
    """14 frames through a 10-scan window: the newest scan's logits are bit-identical to MOS4DNet.forward on the node's
    vstack of the same window, labels / filtered rows / metrics equal the node's, and within 2e-4 of the oracle."""
    from sps_amd.baseline_filters import MOS4DFilter
    p, m = mos4d
    f = MOS4DFilter(m, buffer_size=10, first_index=first_index)
    window = []
    for k in range(14):
        scan = _scan(100 + k, dtype=dtype)
        T = _pose(k)
        res = f(scan, T)
        tr = util.transform_point_cloud(scan[:, :3].astype(np.float64), T)
        window = (window + [(first_index + k, tr)])[-10:]
        rows = mos4d_window_rows([w[1] for w in window], [w[0] for w in window])
        assert res.scan_index == first_index + k and res.window == [w[0] for w in window]
        np.testing.assert_array_equal(res.transformed.cpu().numpy(), tr.astype(np.float32))
        want = m(torch.from_numpy(rows).cuda())[-len(scan):]
        assert torch.equal(res.logits, want), k
        pred = (want > 0).int().cpu().numpy()
        np.testing.assert_array_equal(res.labels.cpu().numpy(), pred.astype(np.float32))
        s32 = scan.astype(np.float32)
        np.testing.assert_array_equal(res.filtered.cpu().numpy(), np.c_[s32[pred == 0, :3], np.zeros((pred == 0).sum())])
        gt = np.where(s32[:, 3] < np.float32(0.84), 0, 1)
        want_m = util.calculate_metrics(gt, pred)
        np.testing.assert_allclose([res.precision, res.recall, res.F1, res.accuracy, res.dIoU], want_m, rtol=1e-12)
        assert res.counts["count"] == len(scan) and res.t_total > 0 and res.t_infer > 0
    ref, _ = O.head_forward(p, rows, 0.2)
    np.testing.assert_allclose(res.logits.cpu().numpy(), ref[-len(scan):, 2], rtol=0, atol=2e-4)


def test_mos4d_filter_off_keeps_everything(mos4d):
    from sps_amd.baseline_filters import MOS4DFilter
    f = MOS4DFilter(mos4d[1], buffer_size=3, filter=False)
    for k in range(4):
        scan = _scan(200 + k)
        res = f(scan, _pose(k))
        assert (res.labels == 0).all() and (res.logits == 0).all()
        np.testing.assert_array_equal(res.filtered.cpu().numpy(), np.c_[scan[:, :3], np.zeros(len(scan), np.float32)])


# ---- MapMOS ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("map_dtype", [np.float64, np.float32])
def test_mapmos_filter_matches_predict(mapmos, map_dtype):
    """Crop == the node's select_points_within_radius; logits bit-identical to MapMOSNet.predict(scan, crop, ones,
    zeros); filtered == scan[labels == 0]; empty crop, empty scan, capacity overflow reported then recovered."""
    from sps_amd.baseline_filters import MapMOSFilter
    _, m = mapmos
    mp = synthetic.build_map(offsets=(-30.0, 0.0, 30.0), n_beams=32, n_azimuth=200)[:, :3].astype(map_dtype)
    f = MapMOSFilter(m, mp)
    for k, scan_dtype in ((0, np.float32), (1, np.float64), (2, np.float32)):
        scan = _scan(300 + k, n_az=200, dtype=scan_dtype)
        T = _pose(3 * k)
        res = f(scan, T)
        sel = crop_indices(mp, T[:3, 3], 30.0)
        assert res.n_map == len(sel) > 0
        crop32 = mp[sel].astype(np.float32)
        np.testing.assert_array_equal(res.crop.cpu().numpy(), crop32)
        s32 = torch.from_numpy(util.transform_point_cloud(scan[:, :3].astype(np.float64), T).astype(np.float32)).cuda()
        c32 = torch.from_numpy(crop32).cuda()
        ls, lm = m.predict(s32, c32, torch.ones(len(s32), 1, device="cuda"), torch.zeros(len(c32), 1, device="cuda"))
        assert torch.equal(res.logits_scan, ls) and torch.equal(res.logits_map, lm)
        lab = m.to_label(ls).cpu().numpy()
        np.testing.assert_array_equal(res.labels.cpu().numpy(), lab)
        np.testing.assert_array_equal(res.filtered.cpu().numpy(),
                                      np.c_[scan[lab == 0, :3].astype(np.float32), np.zeros((lab == 0).sum(), np.float32)])
    far = np.eye(4)
    far[:3, 3] = [5000.0, 0.0, 0.0]                      # empty crop
    scan = _scan(310, n_az=200)
    res = f(scan, far)
    assert res.n_map == 0 and res.crop.shape == (0, 3)
    sf = torch.from_numpy(util.transform_point_cloud(scan[:, :3].astype(np.float64), far).astype(np.float32)).cuda()
    ls, _ = m.predict(sf, torch.empty((0, 3), device="cuda"), torch.ones(len(sf), 1, device="cuda"),
                      torch.zeros(0, 1, device="cuda"))
    assert torch.equal(res.logits_scan, ls)
    res = f(np.zeros((0, 4), np.float32), _pose(0))     # empty scan: map feature 1 (i_min == i_max)
    sel = crop_indices(mp, _pose(0)[:3, 3], 30.0)
    c32 = torch.from_numpy(mp[sel].astype(np.float32)).cuda()
    _, lm = m.predict(torch.empty((0, 3), device="cuda"), c32, torch.ones(0, 1, device="cuda"),
                      torch.zeros(len(c32), 1, device="cuda"))
    assert res.logits_scan.shape == (0,) and res.filtered.shape == (0, 4) and torch.equal(res.logits_map, lm)
    small = MapMOSFilter(m, mp, crop_capacity=100)
    with pytest.raises(SpsError) as ei:
        small(scan, _pose(0))
    assert ei.value.code == ERR_ITEMCAP
    assert small(scan, far).n_map == 0                   # the next frame is clean


# ---- mask --------------------------------------------------------------------------------------------------------------
def test_mask_filter_matches_prune_and_inverse_transform():
    from sps_amd.baseline_filters import MaskFilter
    mp = synthetic.build_map(n_azimuth=300, n_beams=32)
    f = MaskFilter(mp, voxel_size=0.1)
    for k, dtype in ((0, np.float64), (1, np.float32)):
        T = _pose(k + 1)
        world = synthetic.lidar_scan(500 + k, x_offset=0.5 * k, n_azimuth=300, n_beams=32)[:, :3].astype(np.float64)
        scan = util.inverse_transform_point_cloud(world, T).astype(dtype)
        res = f(scan, T)
        w32 = util.transform_point_cloud(scan.astype(np.float64), T).astype(np.float32)
        sub, n_sv = O.prune(O.to_coords(mp[:, :3], 0.1), O.to_coords(w32, 0.1), 0.1)
        assert (res.n_scan_voxels, res.n_submap_voxels) == (n_sv, len(sub)) and len(sub) > 0
        got_sub = res.submap.cpu().numpy()
        np.testing.assert_array_equal(np.unique(got_sub, axis=0), np.unique(sub, axis=0))
        want = util.inverse_transform_point_cloud(got_sub, T).astype(np.float32)          # mask.py:118-123
        np.testing.assert_array_equal(res.filtered.cpu().numpy(), np.c_[want, np.ones(len(want), np.float32)])
        ref = util.inverse_transform_point_cloud(sub, T).astype(np.float32)
        np.testing.assert_array_equal(np.unique(res.filtered[:, :3].cpu().numpy(), axis=0), np.unique(ref, axis=0))


# ---- all three: in flight, ownership, errors ---------------------------------------------------------------------------
def _filters(mos4d, mapmos):
    from sps_amd.baseline_filters import MapMOSFilter, MaskFilter, MOS4DFilter
    mp = synthetic.build_map(offsets=(-20.0, 0.0, 20.0), n_beams=32, n_azimuth=200)
    return {"mos4d": lambda: MOS4DFilter(mos4d[1], buffer_size=4),
            "mapmos": lambda: MapMOSFilter(mapmos[1], mp[:, :3]),
            "mask": lambda: MaskFilter(mp, voxel_size=0.1)}


def _arrays(res):
    return {k: v.cpu().numpy().copy() for k, v in vars(res).items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("name", ["mos4d", "mapmos", "mask"])
def test_frames_in_flight_ownership_and_errors(mos4d, mapmos, name):
    """Three frames submitted back to back without synchronisation give the results of three synchronous frames; a result
    is not overwritten by later submits; a far-out coordinate raises SpsError at result() and the next frame is clean."""
    make = _filters(mos4d, mapmos)[name]
    scans = [_scan(600 + k, n_az=200) for k in range(3)]
    poses = [_pose(k) for k in range(3)]
    sync = make()
    want = [_arrays(sync(s, T)) for s, T in zip(scans, poses)]
    f = make()
    pend = [f.submit(s, T) for s, T in zip(scans, poses)]
    got = [pd.result() for pd in pend]
    first = got[0]
    for _ in range(3):
        f(scans[2], poses[2])                                        # later frames reuse nothing of earlier ones
    for g, w in zip(got, want):
        a = _arrays(g)
        assert a.keys() == w.keys()
        for k in w:
            np.testing.assert_array_equal(a[k], w[k], err_msg=f"{name}.{k}")
    assert _arrays(first).keys() == want[0].keys()
    bad = scans[1].copy()
    bad[0, 0] = 3.0e4
    with pytest.raises(SpsError):
        f(bad, poses[1])
    after = f(scans[0], poses[0])
    if name != "mos4d":                                              # (4DMOS: a different window from the first run)
        for k, v in _arrays(after).items():
            np.testing.assert_array_equal(v, want[0][k], err_msg=f"{name}.{k}")
    else:
        assert bad[0, 0] not in after.transformed[:, 0].cpu().numpy()
