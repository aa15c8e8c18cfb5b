"""LTS baseline on the MI355X: projection, SPCTReg forward and the online filter against the restatement
(tests/lts_reference.py, itself pinned to the reference's outputs by tests/test_lts_cpu.py)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests.lts_reference import lidar_dims, lts_forward, lts_metrics, lts_project, lts_windows
from tests.lts_weights import HEAD_BIAS, lts_cloud, lts_state_dict

pytestmark = pytest.mark.gpu
EPS = 0.84


def _model(lidar="hdl-32", qk_differ=False):
    from sps_amd.models.lts import SPCTReg
    m = SPCTReg()
    m.load_state_dict(lts_state_dict(head_bias=HEAD_BIAS[lidar], qk_differ=qk_differ))
    return m.cuda().eval()


# ---- projection ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lidar,seed", [("hdl-32", 21), ("vlp-16", 22), ("hdl-32", 23)])
def test_projection_is_exact_away_from_bin_edges(lidar, seed):
    from sps_amd.datasets.lts_loader import Loader
    cloud = lts_cloud(lidar, seed, n_rays=30000)
    ref, _ = lts_project(cloud, lidar)
    ld = Loader(torch.from_numpy(cloud).cuda(), lidar)
    assert ld.frame.dtype == np.float32 and ld.frame.shape == ref.shape
    np.testing.assert_array_equal(ld.frame, ref)
    beams, w, nw, N = lidar_dims(lidar)
    assert (ld.num_slices, ld.window_size, ld.num_windows, len(ld)) == (1024, w, nw, nw)
    xr, lr = lts_windows(ref, lidar)
    for i in (0, nw - 1):
        p, l = ld[i]
        np.testing.assert_array_equal(p, xr[i].T)
        np.testing.assert_array_equal(l, lr[i])
    np.testing.assert_array_equal(ld.x_dev.cpu().numpy(), xr)


def test_projection_random_clouds_differ_only_at_bin_edges():
    from sps_amd.datasets.lts_loader import Loader
    for lidar, seed in (("hdl-32", 31), ("vlp-16", 32)):
        cloud = lts_cloud(lidar, seed, n_rays=30000, centred=False)
        ref, pre = lts_project(cloud, lidar)
        got = Loader(torch.from_numpy(cloud).cuda(), lidar).frame
        diff = np.flatnonzero(np.any(got.reshape(-1, 4) != ref.reshape(-1, 4), axis=1))
        if len(diff) == 0:
            continue
        # every differing cell holds (in one of the two results) a row whose pre-floor index is within 1e-4 of an integer
        edge = np.any(np.abs(pre - np.round(pre)) < 1e-4, axis=1)
        d = cloud[cloud[:, 3] != -1]
        edge_rows = {tuple(r) for r in d[edge]}
        for c in diff:
            assert tuple(got.reshape(-1, 4)[c]) in edge_rows or tuple(ref.reshape(-1, 4)[c]) in edge_rows, c
        assert len(diff) < 0.01 * np.count_nonzero(np.any(ref != 0, axis=-1))


def test_projection_errors_and_empty_cloud():
    from sps_amd.datasets.lts_loader import Loader
    base = lts_cloud("hdl-32", 41, n_rays=100)
    for p in ([10.0, 0.0, 12.0, 0.5], [10.0, 0.0, -30.0, 0.5], [np.nan, 1.0, 0.0, 0.5]):
        with pytest.raises(IndexError):
            Loader(torch.from_numpy(np.r_[base, np.array([p], np.float32)]).cuda(), "hdl-32")
    ok = Loader(torch.from_numpy(base).cuda(), "hdl-32")                 # the status was cleared
    np.testing.assert_array_equal(ok.frame, lts_project(base, "hdl-32")[0])
    empty = Loader(torch.zeros((0, 4)).cuda(), "vlp-16")
    assert empty.frame.shape == (16, 1024, 4) and not empty.frame.any()


# ---- forward ---------------------------------------------------------------------------------------------------------
_X = {}


def _inputs(B, N):
    key = (B, N)
    if key not in _X:
        fr, _ = lts_project(lts_cloud("hdl-32", 50, n_rays=60000), "hdl-32")
        x, _ = lts_windows(fr, "hdl-32")                              # [16, 3, 2048]
        xx = np.concatenate([x, x[:, :, ::-1]], axis=0)[:B, :, :N]
        _X[key] = np.ascontiguousarray(xx)
    return _X[key]


@pytest.mark.parametrize("B", [1, 8, 16])
@pytest.mark.parametrize("N", [2048, 1000, 1])
def test_forward_matches_f64_restatement(B, N):
    model = _model()
    x = _inputs(B, N)
    taps = {}
    got = model(torch.from_numpy(x).cuda(), taps=taps)
    assert got.shape == (B, 1, N)
    got = got[:, 0].cpu().numpy()
    ref, rtaps = lts_forward(model.state_dict(), x, torch.float64, device="cuda")
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4)
    for k in ("embedding", "sa1", "sa2", "sa3", "sa4", "max", "mean"):
        t = taps[k].cpu().numpy()
        assert t.shape == rtaps[k].shape, k
        np.testing.assert_allclose(t, rtaps[k], rtol=0, atol=1e-4 * np.abs(rtaps[k]).max(), err_msg=k)
    band = np.abs(ref - EPS) > 1e-5
    np.testing.assert_array_equal((got < np.float32(EPS))[band], (ref < EPS)[band])
    if N == 2048 and B >= 8:
        assert 0.05 < float((ref >= EPS).mean()) < 0.95


def test_forward_golden_and_shared_qk_checkpoint():
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "lts_forward.npz"))
    x = torch.from_numpy(g["x"]).cuda()
    np.testing.assert_allclose(_model()(x)[:, 0].cpu().numpy(), g["scores"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(_model(qk_differ=True)(x)[:, 0].cpu().numpy(), g["scores_qk"], rtol=0, atol=1e-4)


def test_forward_is_bit_reproducible():
    model = _model()
    x = torch.from_numpy(_inputs(16, 2048)).cuda()
    a = model(x).cpu().numpy()
    model(torch.from_numpy(_inputs(8, 1000)).cuda())                   # another shape in between
    b = model(x).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- online filter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lidar", ["hdl-32", "vlp-16"])
def test_filter_is_stream_ordered_and_matches_restatement(lidar):
    from sps_amd.lts_filter import LTSFilter
    f = LTSFilter(_model(lidar), lidar=lidar, epsilon_1=EPS)
    clouds = [lts_cloud(lidar, 60 + i, n_rays=20000 + 5000 * i) for i in range(3)]
    pending = [f.submit(torch.from_numpy(c).cuda()) for c in clouds]   # three frames in flight, nothing synchronised
    any_kept = any_dropped = False
    for c, pend in zip(clouds, pending):
        res = pend.result()
        frame, _ = lts_project(c, lidar)
        x, labels = lts_windows(frame, lidar)
        ref, _ = lts_forward(f.model.state_dict(), x, torch.float64, device="cuda")
        ref = ref.reshape(-1)
        got = res.scores.cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4)
        np.testing.assert_array_equal(res.labels.cpu().numpy(), labels.reshape(-1))
        pts = x.transpose(0, 2, 1).reshape(-1, 3)
        np.testing.assert_array_equal(res.points.cpu().numpy(), pts)
        keep = got <= np.float32(EPS)
        band = np.abs(ref - EPS) > 1e-5
        np.testing.assert_array_equal(keep[band], (ref <= EPS)[band])
        np.testing.assert_array_equal(res.filtered.cpu().numpy(), np.c_[pts, got][keep])   # empty cells included
        m = lts_metrics(got, labels, EPS)                              # same scores -> same counts and ratios
        for k in ("precision", "recall", "accuracy", "dIoU"):
            assert abs(getattr(res, k) - m[k]) < 1e-12, (k, getattr(res, k), m[k])
        assert abs(res.F1 - m["f1"]) < 1e-12
        assert abs(res.loss - m["loss"]) < 1e-6 and abs(res.r2 - m["r2"]) < 1e-6
        assert res.counts["count"] == len(got) and res.counts["tp"] == m["tp"] and res.counts["tn"] == m["tn"]
        assert res.t_project > 0 and res.t_infer > 0 and res.t_filter > 0
        any_kept |= bool(keep.any())
        any_dropped |= bool((~keep).any())
    assert any_kept and any_dropped
    bad = np.r_[clouds[0], np.array([[10.0, 0.0, 12.0, 0.5]], np.float32)] if lidar == "hdl-32" else \
        np.r_[clouds[0], np.array([[10.0, 0.0, 9.0, 0.5]], np.float32)]
    with pytest.raises(IndexError):
        f(torch.from_numpy(bad).cuda())
    f(torch.from_numpy(clouds[0]).cuda())                             # the status was cleared
