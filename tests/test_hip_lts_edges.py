"""The LTS forward (sps_amd/csrc/lts_kernels.inc.h) where its suite was thin: every tile edge of the 32-key / 32-query
attention tiles and the 128 x 128 GEMM tiles, the pass-B split count, a softmax whose running maximum rises late and
by a lot, rows at very different maxima, pooled columns that are negative at every point, and the shape limits.
Everything is compared with the f64 restatement (tests/lts_reference.py), scores and every tap; the conditions the
peaked and negative-pool cases rest on are asserted on that restatement by tests/test_lts_cpu.py."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests.lts_reference import lts_forward
from tests.lts_weights import (HEAD_BIAS, NEG_POOL_BIAS, NEG_POOL_CHANNELS, NEG_POOL_SHAPES, PEAKED_QK_GAIN, PEAKED_SHAPE,
                               lts_dup_inputs, lts_dup_rows, lts_inputs, lts_state_dict)

pytestmark = pytest.mark.gpu
TAPS = ("embedding", "sa1", "sa2", "sa3", "sa4", "max", "mean")
CANARY = -7.0                                 # no score (a sigmoid) and no pad of a tap buffer holds it by accident
_MODELS, _REFS = {}, {}


def _model(kind="plain"):
    if kind not in _MODELS:
        from sps_amd.models.lts import SPCTReg
        kw = {"plain": {}, "peaked": dict(qk_gain=PEAKED_QK_GAIN),
              "negpool": dict(linear1_bn_bias_override={c: NEG_POOL_BIAS for c in NEG_POOL_CHANNELS})}[kind]
        m = SPCTReg()
        m.load_state_dict(lts_state_dict(head_bias=HEAD_BIAS["hdl-32"], **kw))
        _MODELS[kind] = m.cuda().eval()
    return _MODELS[kind]


def _run(model, x):
    """Scores [B, N] and taps of the HIP forward, as numpy."""
    taps = {}
    got = model(torch.from_numpy(x).cuda(), taps=taps)
    assert got.shape == (x.shape[0], 1, x.shape[2])
    return got[:, 0].cpu().numpy(), {k: v.cpu().numpy() for k, v in taps.items()}


def _assert_close(got, gtaps, ref, rtaps, tol=None, what=""):
    """Scores within atol 1e-4 and each tap within 1e-4 max|ref| of the f64 restatement (the forward test's
    tolerances), or within tol[name] where a case derives its own."""
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=0, atol=tol["scores"] if tol else 1e-4, err_msg=f"{what} scores")
    for k in TAPS:
        assert gtaps[k].shape == rtaps[k].shape, k
        assert np.isfinite(gtaps[k]).all(), k
        atol = tol[k] if tol else 1e-4 * np.abs(rtaps[k]).max()
        np.testing.assert_allclose(gtaps[k], rtaps[k], rtol=0, atol=atol, err_msg=f"{what} {k}")


# ---- 1. tile edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 2047, 2049])
def test_tile_edge_sizes_match_f64_and_write_nothing_past_the_last_row(B, N):
    """N around the 32-row attention tiles, the 128-row GEMM tiles and the 2048-point window: scores and every tap
    against f64; then the same forward through the raw handle into buffers with a canary-filled tail: the output
    has B * N rows (taps: B * N or B) and nothing is written behind them."""
    model = _model()
    x = lts_inputs(B, N)
    assert x.shape == (B, 3, N)
    got, gtaps = _run(model, x)
    ref, rtaps = lts_forward(model.state_dict(), x, torch.float64, device="cuda")
    _assert_close(got, gtaps, ref, rtaps, what=f"B={B} N={N}")

    h = model.handle(0)
    st = torch.cuda.current_stream().cuda_stream
    xd = torch.from_numpy(x).cuda()
    pad = 256
    buf = torch.full((B * N + pad,), CANARY, dtype=torch.float32, device="cuda")
    h.forward(xd.data_ptr(), B, N, buf.data_ptr(), st)
    raw = buf.cpu().numpy()
    assert (raw[B * N:] == np.float32(CANARY)).all(), "scores were written past row B * N"
    np.testing.assert_allclose(raw[: B * N].reshape(B, N), ref, rtol=0, atol=1e-4)
    for i, name in enumerate(TAPS):
        r, c = h.tap_shape(i)
        assert (r, c) == ((B * N, 128) if i < 5 else (B, 2048)), name
        t = torch.full((r * c + pad,), CANARY, dtype=torch.float32, device="cuda")
        h.tap(i, t.data_ptr(), st)
        t = t.cpu().numpy()
        assert (t[r * c:] == np.float32(CANARY)).all(), f"tap {name} was written past its last row"
        tt = t[: r * c].reshape(B, N, c).transpose(0, 2, 1) if i < 5 else t[: r * c].reshape(B, c)
        np.testing.assert_allclose(tt, rtaps[name], rtol=0, atol=1e-4 * np.abs(rtaps[name]).max(), err_msg=name)


# ---- 2. pass-B split count ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1000, 2048])
def test_window_zero_does_not_depend_on_the_split_count(N):
    """One window as window 0 of B = 1, 2 and 16 (the other windows hold other data).  The host splits the query axis
    of pass B by ktiles = ceil(N / 32), splits = min(8, max(1, 2048 / (B ktiles)), ktiles), rows_per_split =
    32 ceil(ktiles / splits), splits = ceil(N / rows_per_split):
        N = 1000 (ktiles 32): B = 1 -> 8 splits of 128 rows, B = 2 -> 8 of 128, B = 16 -> 4 of 256
        N = 2048 (ktiles 64): B = 1 -> 8 splits of 256 rows, B = 2 -> 8 of 256, B = 16 -> 2 of 1024
    Window 0 matches f64 at the forward test's tolerances in every run, and the runs agree within twice that."""
    model = _model()
    x1 = lts_inputs(1, N)
    ref, rtaps = lts_forward(model.state_dict(), x1, torch.float64, device="cuda")
    runs = {}
    for B in (1, 2, 16):
        x = lts_inputs(B, N)
        assert np.array_equal(x[0], x1[0]) and all(not np.array_equal(x[b], x1[0]) for b in range(1, B))
        got, gtaps = _run(model, x)
        runs[B] = (got[:1], {k: v[:1] for k, v in gtaps.items()})
        _assert_close(*runs[B], ref, rtaps, what=f"B={B}")
    for a, b in ((1, 2), (1, 16), (2, 16)):
        np.testing.assert_allclose(runs[a][0], runs[b][0], rtol=0, atol=2e-4, err_msg=f"B={a} against B={b}")
        for k in TAPS:
            np.testing.assert_allclose(runs[a][1][k], runs[b][1][k], rtol=0, atol=2e-4 * np.abs(rtaps[k]).max(),
                                       err_msg=f"{k}: B={a} against B={b}")


# ---- 3 / 4. peaked softmax ------------------------------------------------------------------------------------------
def _peaked_reference(name, x):
    """f64 restatement of the peaked model on x and the tolerance of the case: per tap and for the scores,
    max(the forward test's tolerance, 4 x the restatement's own f32 error on this input); 4 covers another summation
    order and __expf against exp.  Computed on the CPU (the same figures with and without a GPU) and printed."""
    if name not in _REFS:
        sd = lts_state_dict(qk_gain=PEAKED_QK_GAIN)
        ref, rtaps = lts_forward(sd, x, torch.float64, probes=True)
        s32, t32 = lts_forward(sd, x, torch.float32)
        base = {"scores": 1e-4, **{k: 1e-4 * float(np.abs(rtaps[k]).max()) for k in TAPS}}
        err = {"scores": float(np.abs(s32 - ref).max()), **{k: float(np.abs(t32[k] - rtaps[k]).max()) for k in TAPS}}
        tol = {k: max(base[k], 4.0 * err[k]) for k in base}
        for k in base:
            print(f"lts edge tests, {name}: {k:9s} f32 restatement error {err[k]:.3e}  forward-test tolerance "
                  f"{base[k]:.3e}  allowed {tol[k]:.3e}")
        _REFS[name] = (ref, rtaps, tol)
    return _REFS[name]


def test_peaked_softmax_matches_f64():
    """qk_gain = 0.35 * 4: in every attention layer a quarter of the rows have max - median energy >= 30 and the
    arg-max key of most rows lies past the first key tile (tests/test_lts_cpu.py asserts both), so pass A's
    rescale of the running sum and the merge of the two half-waves carry weight."""
    x = lts_inputs(*PEAKED_SHAPE)
    ref, rtaps, tol = _peaked_reference("peaked softmax", x)
    got, gtaps = _run(_model("peaked"), x)
    _assert_close(got, gtaps, ref, rtaps, tol, "peaked")


def test_tied_rows_and_spread_rows_in_one_window_match_f64():
    """Half of each window one point repeated (identical q rows, exactly tied energies), half spread points, under the
    peaked model: no NaN, f64 agreement, and explicitly on the repeated rows and on the keys whose column sum is
    below the 1e-9 of k_lts_attn_combine's denominator (there the floor, not the sum, sets x_r)."""
    x = lts_dup_inputs()
    ref, rtaps, tol = _peaked_reference("tied and spread rows", x)
    got, gtaps = _run(_model("peaked"), x)
    assert not np.isnan(got).any() and not any(np.isnan(v).any() for v in gtaps.values())
    _assert_close(got, gtaps, ref, rtaps, tol, "tied")
    floor_rows = 0
    for b in range(x.shape[0]):
        rows = lts_dup_rows(b)
        np.testing.assert_allclose(got[b, rows], ref[b, rows], rtol=0, atol=tol["scores"], err_msg="repeated rows")
        for layer in range(1, 5):
            k = f"sa{layer}"
            np.testing.assert_allclose(gtaps[k][b][:, rows], rtaps[k][b][:, rows], rtol=0, atol=tol[k],
                                       err_msg=f"{k}, repeated rows of window {b}")
            floor = rtaps[f"colsum{layer}"][b] < 1e-9
            floor_rows += int(floor.sum())
            np.testing.assert_allclose(gtaps[k][b][:, floor], rtaps[k][b][:, floor], rtol=0, atol=tol[k],
                                       err_msg=f"{k}, keys under the denominator floor of window {b}")
    assert floor_rows > 0


# ---- 5. all-negative pool columns -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", NEG_POOL_SHAPES)
def test_pool_of_all_negative_columns(B, N):
    """linear1's BN beta is -20 on the first / last column of a lane group, a wave, a 128-tile and the tensor: every
    pre-activation of those columns is < -1 (tests/test_lts_cpu.py), so their max is 0.2 v < 0 and any zero of a
    padded row of the last 128-row tile that got into the max, or any other divisor than N in the mean, shows."""
    model = _model("negpool")
    x = lts_inputs(B, N)
    got, gtaps = _run(model, x)
    ref, rtaps = lts_forward(model.state_dict(), x, torch.float64, device="cuda")
    ch = list(NEG_POOL_CHANNELS)
    assert (rtaps["max"][:, ch] < -0.2).all()
    assert (gtaps["max"][:, ch] < 0).all(), gtaps["max"][:, ch]
    for k in ("max", "mean"):
        np.testing.assert_allclose(gtaps[k][:, ch], rtaps[k][:, ch], rtol=0, atol=1e-4 * np.abs(rtaps[k]).max(), err_msg=k)
    _assert_close(got, gtaps, ref, rtaps, what=f"N={N}")


# ---- 6. shape limits ---------------------------------------------------------------------------------------------------
def test_bad_shapes_raise_before_anything_runs_and_leave_the_handle_usable():
    """sps_lts_forward tests the shape right after its null checks, before it touches the device or either pointer, so
    the shapes are passed with the pointers of two small buffers; the score buffer keeps its canary and the handle's
    taps still belong to the forward before.  Then the golden forward on the same handle."""
    from sps_amd import _native
    model = _model()
    h = model.handle(0)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(lts_inputs(2, 33)).cuda()
    model(x)
    assert h.tap_shape(0) == (66, 128)
    buf = torch.full((1024,), CANARY, dtype=torch.float32, device="cuda")
    max_points = 1 << 23                                               # SPS_MAX_POINTS (include/sps_hip.h)
    bad = [(0, 33), (2, 0), (-1, 33), (2, -1), (65536, 1), (1, (1 << 20) + 1), (8193, 1024), (9, 932068)]
    assert all(B * N > max_points and B <= 65535 and N <= 1 << 20 for B, N in bad[-2:])
    for B, N in bad:
        with pytest.raises(_native.SpsError, match=f"bad shape B={B} N={N}") as e:
            h.forward(x.data_ptr(), B, N, buf.data_ptr(), st)
        assert e.value.code == _native.ERR_INVALID
    torch.cuda.synchronize()
    assert (buf == CANARY).all()
    assert h.tap_shape(0) == (66, 128)
    for shape in ((0, 3, 33), (2, 3, 0)):                              # through the module: empty tensors
        with pytest.raises(_native.SpsError) as e:
            model(torch.zeros(shape, device="cuda"))
        assert e.value.code == _native.ERR_INVALID
    assert model.handle(0) is h
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "lts_forward.npz"))
    np.testing.assert_allclose(model(torch.from_numpy(g["x"]).cuda())[:, 0].cpu().numpy(), g["scores"], rtol=0, atol=1e-4)
