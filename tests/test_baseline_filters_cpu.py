"""CPU tests of the online 4DMOS / MapMOS / mask filters (sps_amd/baseline_filters.py): checkpoint loading, window
bookkeeping, argument validation, the crop golden and the native symbols.  No GPU needed."""
import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from tests.baseline_reference import crop_golden, crop_indices, mos4d_window_rows
from tests.helpers import state_dict_from_params


def test_crop_golden_reproduced_by_numpy_restatement():
    """The restatement the GPU test compares against selects exactly the reference node's indices, on both map dtypes,
    including the points placed on the 30 m sphere and 1 ulp inside / outside it."""
    maps, poses, r = crop_golden()
    assert r == 30.0 and len(poses) >= 3
    for tag, (m, sels) in maps.items():
        assert m.dtype == (np.float64 if tag == "64" else np.float32)
        for T, sel in zip(poses, sels):
            c = T[:3, 3]
            np.testing.assert_array_equal(crop_indices(m, c, r), sel)
            d = np.sqrt(np.sum((m - c) ** 2, axis=1))
            assert (d == r).sum() >= 6 and ((d > r) & (d < r + 1e-5)).any() and ((d < r) & (d > r - 1e-5)).any()
            assert np.all(d[sel] <= r) and len(sel) == (d <= r).sum()


def test_window_bookkeeping_and_t_base():
    from sps_amd.baseline_filters import ScanWindow, window_t_base
    w = ScanWindow(10)
    for k in range(1, 26):
        idx = w.push(k)
        assert idx == k - 1
        want = list(range(max(0, k - 10), k))
        assert w.indices == want and [p for _, p in w.entries] == [i + 1 for i in want]
        # baselines._t_base: 0 while the indices lie in [-16, 15], else the oldest index
        assert w.t_base == (0.0 if k <= 16 else float(k - 10))
    w = ScanWindow(4, first_index=1234)
    for _ in range(6):
        w.push()
    assert w.indices == [1236, 1237, 1238, 1239] and w.t_base == 1236.0
    w.discard(1238)
    assert w.indices == [1236, 1237, 1239]
    assert window_t_base([]) == 0.0 and window_t_base([-16, 15]) == 0.0 and window_t_base([-17, 0]) == -17.0
    # the same rule as the model's own re-basing, on the rows the node would build
    from sps_amd.models.baselines import _t_base
    for idx in ([0, 1, 2], [7, 8, 9, 10, 11, 12, 13, 14, 15, 16], [1234, 1235]):
        rows = mos4d_window_rows([np.zeros((3, 3))] * len(idx), idx)
        assert _t_base(torch.from_numpy(rows)) == window_t_base(idx)


def test_buffer_size_from_checkpoint_name():
    from sps_amd.baseline_filters import MOS4DFilter, buffer_size_from_path
    assert buffer_size_from_path("/sps/c_ws/src/mos4d/checkpoints/10_scans.ckpt") == 10
    assert buffer_size_from_path("ckpt/5_scans.ckpt") == 5
    for bad in ("mos4d.ckpt", "10_scans.pt", "scans.ckpt"):
        with pytest.raises(ValueError, match="buffer size not found"):
            buffer_size_from_path(bad)
        with pytest.raises(ValueError, match="buffer size not found"):
            MOS4DFilter.from_checkpoint(bad)


@pytest.mark.parametrize("prefix,oc,voxel", [("model.MinkUNet.", 3, 0.2), ("mos.MinkUNet.", 1, 0.1)])
def test_checkpoint_state_dict_loads(tmp_path, prefix, oc, voxel):
    """load_model of the nodes: prefix stripped, MOSLoss keys dropped, the rest loads into the network unchanged."""
    from sps_amd.baseline_filters import load_state_dict
    from sps_amd.models.baselines import MapMOSNet, MOS4DNet
    p = O.random_params(seed=9, out_channels=oc)
    sd = state_dict_from_params(p, prefix=prefix)
    sd["MOSLoss.weight"] = torch.ones(3)
    path = tmp_path / "10_scans.ckpt"
    torch.save({"state_dict": sd, "epoch": 3}, path)
    got = load_state_dict(str(path), prefix)
    assert not any("MOSLoss" in k or k.startswith(prefix) for k in got)
    assert set(got) == {k[len(prefix):] for k in sd if "MOSLoss" not in k}
    m = MOS4DNet(voxel) if oc == 3 else MapMOSNet(voxel)
    m.MinkUNet.load_state_dict(got)
    np.testing.assert_array_equal(m.MinkUNet.state_dict()["final.bias"].numpy(), p["final.bias"])


def test_argument_validation():
    from sps_amd.baseline_filters import MapMOSFilter, MaskFilter, MOS4DFilter, _pose, _scan_input
    from sps_amd.models.baselines import MapMOSNet, MOS4DNet
    m4 = MOS4DNet(0.2)
    for bad in (0, 17, 33, 2.5):
        with pytest.raises(ValueError, match="buffer_size"):
            MOS4DFilter(m4, buffer_size=bad)
    with pytest.raises(TypeError):
        MOS4DFilter(MapMOSNet(0.1))
    with pytest.raises(TypeError):
        MapMOSFilter(m4, np.zeros((4, 3)))
    with pytest.raises(ValueError, match="radius"):
        MapMOSFilter(MapMOSNet(0.1), np.zeros((4, 3)), radius=float("nan"))
    with pytest.raises(ValueError, match="crop_capacity"):
        MapMOSFilter(MapMOSNet(0.1), np.zeros((4, 3)), crop_capacity=-1)
    with pytest.raises(ValueError, match="map_points"):
        MapMOSFilter(MapMOSNet(0.1), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="voxel_size"):
        MaskFilter(np.zeros((4, 3)), voxel_size=0.0)
    with pytest.raises(ValueError, match="4x4"):
        _pose(np.eye(3))
    with pytest.raises(ValueError, match=r"\[n, >=3\]"):
        _scan_input(np.zeros((5, 2), np.float32), "cpu", "x")


def test_library_exports_the_baseline_filter_entry_points():
    from sps_amd import _native
    for name in ("sps_forward_head_n", "sps_transform_rows", "sps_transform_points_n", "sps_radius_crop", "sps_label_filter"):
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
    assert _native.lib.sps_version() == 202
    # argument checks of the native entry points (no device work: they fail before touching the GPU)
    assert _native.lib.sps_radius_crop(None, None, 0, 3, 0, None, 30.0, None, 0, None, 5, 0, None, 1.0, None, None) != 0
    assert _native.lib.sps_label_filter(None, None, 1, 0, None, 3, None, 1, None, None, None, None) != 0
    assert _native.lib.sps_forward_head_n(None, None, 5, 0, None, 0.1, None, 0.0, None, 1, 0, None) != 0
