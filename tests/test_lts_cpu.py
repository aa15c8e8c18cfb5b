"""LTS baseline, CPU side: the restatement (tests/lts_reference.py) against the reference's own outputs
(tests/golden/lts_*.npz, tools/capture_lts_goldens.py) and the native blob layout against the reference state_dict."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests.lts_reference import lts_forward, lts_project
from tests.lts_weights import HEAD_BIAS, lts_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


@pytest.mark.parametrize("case", ["hdl32", "vlp16", "hdl32_random"])
def test_restatement_projection_matches_reference(case):
    g = _load(f"lts_proj_{case}.npz")
    frame, _ = lts_project(g["cloud"], str(g["lidar"]))
    flat = frame.reshape(-1, 4)
    cells = np.flatnonzero(np.any(flat != 0, axis=1))
    np.testing.assert_array_equal(cells, g["cells"])
    np.testing.assert_array_equal(flat[cells], g["rows"])


def test_restatement_rejects_what_the_reference_rejects():
    g = _load("lts_proj_errors.npz")
    for cloud in g["bad"]:
        with pytest.raises(IndexError):
            lts_project(cloud, "hdl-32")
    lts_project(g["dropped_ok"], "hdl-32")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restatement_forward_matches_reference(dtype):
    g = _load("lts_forward.npz")
    sd = lts_state_dict(head_bias=HEAD_BIAS["hdl-32"])
    scores, taps = lts_forward(sd, g["x"], dtype)
    np.testing.assert_allclose(scores, g["scores"], rtol=0, atol=1e-5)
    st = int(g["tap_stride"])
    for k in ("embedding", "sa1", "sa2", "sa3", "sa4"):
        ref = g[f"tap_{k}"]
        np.testing.assert_allclose(taps[k][:, :, ::st], ref, rtol=0, atol=1e-5 * np.abs(ref).max())
    for k in ("max", "mean"):
        np.testing.assert_allclose(taps[k], g[f"tap_{k}"], rtol=0, atol=1e-5 * np.abs(g[f"tap_{k}"]).max())
    qk, _ = lts_forward(lts_state_dict(head_bias=HEAD_BIAS["hdl-32"], qk_differ=True), g["x"], dtype)
    np.testing.assert_allclose(qk, g["scores_qk"], rtol=0, atol=1e-5)
    assert 0.1 < float((g["scores"] >= 0.84).mean()) < 0.9          # the weights put scores on both sides of eps


def _golden_keys():
    g = _load("lts_keys.npz")
    return [(str(k), tuple(int(d) for d in s if d >= 0)) for k, s in zip(g["keys"], g["shapes"])]


def test_native_blob_layout_is_the_reference_state_dict():
    from sps_amd import _native
    layout = _native.lts_layout()
    assert [(n, s) for n, _, _, s in layout] == _golden_keys()
    off = 0
    for _, o, numel, shape in layout:
        assert o == off and numel == int(np.prod(shape))
        off += numel
    assert off == _native.lib.sps_lts_numel()
    assert _native.lib.sps_version() == _native.ABI_VERSION == 202


def test_spctreg_state_dict_keys_and_reference_checkpoint_load():
    from sps_amd.models.lts import SPCTReg
    m = SPCTReg()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == _golden_keys()
    sd = lts_state_dict(qk_differ=True)
    m.load_state_dict({"model_state_dict": sd}["model_state_dict"])     # what the node does with best_model.pth
    for k in range(1, 5):                                                 # one shared Parameter: k_conv's value wins
        assert m.get_submodule(f"sa{k}").q_conv.weight is m.get_submodule(f"sa{k}").k_conv.weight
        torch.testing.assert_close(m.state_dict()[f"sa{k}.q_conv.weight"], sd[f"sa{k}.k_conv.weight"], rtol=0, atol=0)
    blob = m.pack()
    from sps_amd import _native
    for name, off, numel, _ in _native.lts_layout():
        np.testing.assert_array_equal(blob[off: off + numel], m.state_dict()[name].float().reshape(-1).numpy())


def test_cpu_tensor_raises():
    from sps_amd.models.lts import SPCTReg
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SPCTReg().eval()(torch.zeros(1, 3, 8))


def test_loader_rejects_unknown_lidar():
    from sps_amd.datasets.lts_loader import Loader
    with pytest.raises(AssertionError, match="lidar type should be 'vlp-16' or 'hdl-32'"):
        Loader(np.zeros((1, 4), np.float32), "os-64")
