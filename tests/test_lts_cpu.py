"""LTS baseline, CPU side: the restatement (tests/lts_reference.py) against the reference's own outputs
(tests/golden/lts_*.npz, tools/capture_lts_goldens.py) and the native blob layout against the reference state_dict."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests.lts_reference import lts_forward, lts_project
from tests.lts_weights import (HEAD_BIAS, NEG_POOL_BIAS, NEG_POOL_CHANNELS, NEG_POOL_SHAPES, PEAKED_K, PEAKED_SHAPE,
                               lts_dup_inputs, lts_dup_rows, lts_inputs, lts_state_dict)

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


# ---- what the edge tests of the HIP forward rest on (tests/test_hip_lts_edges.py) -----------------------------------
def test_default_state_dict_bits_are_pinned():
    """lts_state_dict() without its later keyword arguments: the bytes tests/golden/lts_forward.npz was captured with
    (sha256 of the tensors' bytes in state_dict order, taken from the function before it had qk_gain)."""
    import hashlib

    def digest(sd):
        return hashlib.sha256(b"".join(v.numpy().tobytes() for v in sd.values())).hexdigest()

    assert digest(lts_state_dict()) == "b757510e1136ac229d923cb254dc243e4f98c41995c8496d02ee6f8d8542c818"
    assert digest(lts_state_dict(qk_differ=True)) == "98b3d91c0eec88d7344f94f0ba1117174ccb2ed4de8ca206e0d1270e7959e4e9"
    assert digest(lts_state_dict(qk_gain=0.35, linear1_bn_bias_override={})) == digest(lts_state_dict())
    sd, ov = lts_state_dict(), lts_state_dict(qk_gain=0.7, linear1_bn_bias_override={5: -3.0})
    for k in sd:                                   # the two arguments touch the q / k kernels and one beta, nothing else
        if ".q_conv." in k or ".k_conv." in k:
            np.testing.assert_array_equal(ov[k].numpy(), (sd[k].double() / 0.35 * 0.7).float().numpy())   # one rounding
        elif k == "linear1.1.bias":
            assert ov[k][5] == -3.0 and torch.equal(ov[k][:5], sd[k][:5]) and torch.equal(ov[k][6:], sd[k][6:])
        else:
            assert torch.equal(ov[k], sd[k]), k


def _peaked_conditions(k, x):
    """(a), (b), (c) of the peaked-softmax case for qk_gain = 0.35 k on input x, from the f64 restatement alone."""
    scores, taps = lts_forward(lts_state_dict(qk_gain=0.35 * k), x, torch.float64, probes=True)
    a = b = True
    c = bool(np.isfinite(scores).all()) and all(np.isfinite(v).all() for v in taps.values())
    for layer in range(1, 5):
        E = taps[f"energy{layer}"]                                     # [B, query, key]
        a &= float((E.max(-1) - np.median(E, -1) >= 30).mean()) >= 0.25
        b &= float((E.argmax(-1) >= 32).mean()) >= 0.10
        c &= float(np.abs(E).max()) < 3e4
    return a, b, c


def test_peaked_gain_is_the_smallest_that_peaks_every_layer():
    """PEAKED_K is the smallest integer k for which, with qk_gain = 0.35 k, in each of the four attention layers (a) a
    quarter of the query rows have max_j E - median_j E >= 30, (b) a tenth have their arg-max key past the first
    32-key tile (the running maximum of pass A rises late), (c) everything stays finite and |E| < 3e4."""
    x = lts_inputs(*PEAKED_SHAPE)
    for k in range(1, PEAKED_K):
        assert not all(_peaked_conditions(k, x)), k
    assert _peaked_conditions(PEAKED_K, x) == (True, True, True)


def test_duplicate_point_input_ties_and_reaches_the_denominator_floor():
    """lts_dup_inputs() under the peaked model: finite, |E| < 3e4, the repeated rows' energies tie, and in some
    layer key columns of every window sum to less than the 1e-9 of the column normalisation (so the floor decides)."""
    x = lts_dup_inputs()
    for b in range(x.shape[0]):
        assert (x[b][:, lts_dup_rows(b)] == x[b][:, lts_dup_rows(b)][:, :1]).all()
    scores, taps = lts_forward(lts_state_dict(qk_gain=0.35 * PEAKED_K), x, torch.float64, probes=True)
    assert np.isfinite(scores).all() and all(np.isfinite(v).all() for v in taps.values())
    for b in range(x.shape[0]):
        rows = lts_dup_rows(b)
        floor = False
        for layer in range(1, 5):
            E = taps[f"energy{layer}"][b]
            assert np.abs(E).max() < 3e4
            tie = E[rows][:, rows]                 # equal but for the BLAS's blocking (identical q rows on the device)
            assert np.ptp(tie) <= 1e-13 * np.abs(tie).max()
            floor |= bool((taps[f"colsum{layer}"][b] < 1e-9).any())
        assert floor


def test_negative_pool_bias_keeps_every_preactivation_below_minus_one():
    over = {c: NEG_POOL_BIAS for c in NEG_POOL_CHANNELS}
    sd = lts_state_dict(linear1_bn_bias_override=over)
    for B, N in NEG_POOL_SHAPES:
        _, taps = lts_forward(sd, lts_inputs(B, N), torch.float64, probes=True)
        pre = taps["linear1_pre"][:, list(NEG_POOL_CHANNELS)]
        assert pre.shape == (B, len(NEG_POOL_CHANNELS), N) and pre.max() < -1.0, (N, pre.max())
        np.testing.assert_array_equal(taps["max"][:, list(NEG_POOL_CHANNELS)], 0.2 * pre.max(-1))
        assert (taps["max"][:, list(NEG_POOL_CHANNELS)] < 0).all()
        rest = np.setdiff1d(np.arange(2048), NEG_POOL_CHANNELS)
        assert (taps["linear1_pre"][:, rest].max(-1) > 0).mean() > 0.3      # the other columns still see positive values
