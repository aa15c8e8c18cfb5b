"""GPU tests of the ordered compaction (compact_count / compact_base / compact_rank, sps_amd/csrc/aux_kernels.inc.h) under
the native entries that keep rows "in input order, no atomics": sizes on both sides of a wave and of one, two and three
workgroups of 1024 rows, and keep patterns that empty a wave or a whole workgroup between two kept ones.  Every case
states the kept set as a numpy mask, builds an input whose flags are that mask, and asserts the count words, the kept rows
bit for bit in input order, and that nothing behind the last kept row was written."""
import numpy as np
import pytest
import torch

from sps_amd._native import ERR_ITEMCAP, SpsError
from sps_amd.datasets import util
from tests.helpers import CFG

pytestmark = pytest.mark.gpu

EPS = np.float32(CFG["FILTER"]["THRESHOLD"])
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 3073]
PATTERNS = ["none", "all", "first", "last", "alternate", "wave_hole", "block_hole"]
CANARY = np.float32(-12345.5)


def cases(test):
    return pytest.mark.parametrize("n", SIZES)(pytest.mark.parametrize("pattern", PATTERNS)(test))


def stream():
    return torch.cuda.current_stream().cuda_stream


def ctx():
    from sps_amd.models.models import get_context
    return get_context(0, stream())


def keep_mask(pattern, n):
    m = np.zeros(n, bool)
    if pattern in ("all", "wave_hole", "block_hole"):
        m[:] = True
    if pattern == "first":
        m[:1] = True
    if pattern == "last":
        m[-1:] = True
    if pattern == "alternate":
        m[::2] = True
    if pattern == "wave_hole":          # wave 7 of a workgroup: of the second one where there is a third behind it
        lo = (1024 if n >= 2048 else 0) + 448
        m[lo:lo + 64] = False
    if pattern == "block_hole":         # the whole second workgroup
        m[1024:2048] = False
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def canary(*shape, dtype=torch.float32):
    return torch.full(shape, float(CANARY), dtype=dtype, device="cuda")


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64)


def assert_rows(got, want):
    """got[:len(want)] == want bit for bit, and every row behind them still holds the canary"""
    k = len(want)
    np.testing.assert_array_equal(bits(got[:k]), bits(want))
    assert (got[k:] == float(CANARY)).all()


def pick(mask, kept_values, dropped_values, dtype=np.float32):
    """flag operand per row: the values of either list in turn, so that every one of them meets every position"""
    kv, dv = np.asarray(kept_values, dtype), np.asarray(dropped_values, dtype)
    i = np.arange(len(mask))
    return np.where(mask, kv[i % len(kv)], dv[i % len(dv)]).astype(dtype)


def payload(n, cols, seed):
    rows = np.random.default_rng(seed).normal(size=(n, cols)).astype(np.float32)
    rows[3::7, 1] = -0.0
    rows[5::11, 2] = np.nan
    return rows


# ---- sps_compact_stable: k_stable_count / k_stable_write ---------------------------------------------------------------
@cases
def test_compact_stable(n, pattern):
    mask = keep_mask(pattern, n)
    scores = pick(mask, [EPS, np.nextafter(EPS, np.float32(0)), -1.0, 0.0], [np.nextafter(EPS, np.float32(1)), np.nan, 2.0])
    rows = payload(n, 5, 1)                                             # 4 of 5 columns are kept
    out, cnt = canary(n + 2, 4), torch.full((2,), -9, dtype=torch.int32, device="cuda")
    ds, dr = dev(scores), dev(rows)
    ctx().compact_stable(ds.data_ptr(), dr.data_ptr(), 5, 4, n, float(EPS), out.data_ptr(), cnt.data_ptr(), stream())
    assert cnt.tolist() == [int(mask.sum()), -9]
    assert_rows(out, rows[mask, :4])


# ---- sps_label_filter: k_label_count / k_label_write -------------------------------------------------------------------
@cases
def test_label_filter(n, pattern):
    mask = keep_mask(pattern, n)                                        # kept = label 0 = !(logit > 0)
    logits = np.full((n, 3), 7.0, np.float32)
    logits[:, 2] = pick(mask, [0.0, -1.0, np.nan, -0.0], [1.0, np.float32(1e-30), np.inf])
    rows = payload(n, 4, 2)
    rows[:, 3] = pick(np.arange(n) % 3 == 0, [0.84, 1.0], [np.nextafter(np.float32(0.84), np.float32(0)), 0.0])
    lab, out = canary(n + 2), canary(n + 2, 4)
    counts = torch.full((6,), -9, dtype=torch.int32, device="cuda")
    dl, dr = dev(logits), dev(rows)
    ctx().label_filter(dl.data_ptr() + 8, 3, n, dr.data_ptr(), 4, dr.data_ptr() + 12, 4, lab.data_ptr(), out.data_ptr(),
                       counts.data_ptr(), stream())
    pred, gt = ~mask, rows[:, 3] >= np.float32(0.84)
    assert counts.tolist() == [int(mask.sum()), int((gt & pred).sum()), int((~gt & pred).sum()), int((gt & ~pred).sum()),
                               int((~gt & ~pred).sum()), -9]
    assert_rows(lab, pred.astype(np.float32))
    assert_rows(out, np.c_[rows[mask, :3], np.zeros(int(mask.sum()), np.float32)].astype(np.float32).reshape(-1, 4))


# ---- sps_radius_crop: k_crop_count<T> / k_crop_write<T> ----------------------------------------------------------------
R, N_SCAN = 3.0, 5


def crop_map(mask, f64):
    """map points at 0.5 r (kept) and 2 r (dropped) from the pose origin, in random directions"""
    T = np.eye(4)
    T[:3, 3] = [4.0, -2.5, 0.75]
    d = np.random.default_rng(3).normal(size=(len(mask), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = T[:3, 3] + d * np.where(mask, 0.5 * R, 2.0 * R)[:, None]
    return T, np.c_[pts, np.full(len(mask), 55.0)].astype(np.float64 if f64 else np.float32)     # row stride 4


def crop(mp, f64, T, cap, n_rows):
    m = len(mp)
    rows, feats = canary(n_rows, 6), canary(n_rows)
    counts = torch.full((3,), -9, dtype=torch.int32, device="cuda")
    scratch = torch.empty(max(1, -(-m // 1024)), dtype=torch.int32, device="cuda")
    dm = dev(mp)
    ctx().radius_crop(dm.data_ptr(), f64, 4, m, T, R, scratch.data_ptr(), N_SCAN, rows.data_ptr(), 6, cap,
                      feats.data_ptr(), 2.0, counts.data_ptr(), stream())
    return rows, feats, counts.tolist()


def crop_rows(mp, mask):
    want = np.full((int(mask.sum()), 6), CANARY, np.float32)            # column 5 of a row is not the crop's
    want[:, 0], want[:, 1:4], want[:, 4] = 0, mp[mask, :3].astype(np.float32), -1
    return want


@cases
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_radius_crop(n, pattern, f64):
    mask = keep_mask(pattern, n)
    T, mp = crop_map(mask, f64)
    k = int(mask.sum())
    rows, feats, counts = crop(mp, f64, T, n, N_SCAN + n + 2)
    ctx().check_errors(stream())
    assert counts == [k, N_SCAN + k, -9]
    assert (rows[:N_SCAN] == float(CANARY)).all() and (feats[:N_SCAN] == float(CANARY)).all()
    assert_rows(rows[N_SCAN:], crop_rows(mp, mask))
    assert_rows(feats[N_SCAN:], np.full(k, 2.0, np.float32))


@pytest.mark.parametrize("n", [1025, 3073])
@pytest.mark.parametrize("pattern", ["all", "alternate", "block_hole"])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_radius_crop_capacity(n, pattern, f64):
    """cap = kept, kept - 1 and 0: the count saturates, nothing is written at or past n_scan + cap, SPS_ERR_ITEMCAP is
    reported once and the next call is clean"""
    mask = keep_mask(pattern, n)
    T, mp = crop_map(mask, f64)
    kept = int(mask.sum())
    want = crop_rows(mp, mask)
    for cap in (kept, kept - 1, 0):
        rows, feats, counts = crop(mp, f64, T, cap, N_SCAN + kept + 2)
        if cap < kept:
            with pytest.raises(SpsError) as ei:
                ctx().check_errors(stream())
            assert ei.value.code == ERR_ITEMCAP
        ctx().check_errors(stream())
        assert counts == [cap, N_SCAN + cap, -9]
        assert (rows[:N_SCAN] == float(CANARY)).all() and (feats[:N_SCAN] == float(CANARY)).all()
        assert_rows(rows[N_SCAN:], want[:cap])
        assert_rows(feats[N_SCAN:], np.full(cap, 2.0, np.float32))


# ---- sps_filter_finish: k_filter_count / k_filter_write ----------------------------------------------------------------
@cases
@pytest.mark.parametrize("strict", [False, True], ids=["le", "lt"])
def test_filter_finish(n, pattern, strict):
    mask = keep_mask(pattern, n)
    below, above = np.nextafter(EPS, np.float32(0)), np.nextafter(EPS, np.float32(1))
    scores = pick(mask, [below, 0.0, -1.0] + ([] if strict else [EPS]), [above, np.nan, 2.0] + ([EPS] if strict else []))
    raw = payload(n, 6, 4)                                              # whole rows of 5 columns, row stride 6
    out, cnt = canary(n + 2, 5), torch.full((2,), -9, dtype=torch.int32, device="cuda")
    ds, dr = dev(scores), dev(raw)
    ctx().filter_finish(ds.data_ptr(), n, dr.data_ptr(), 6, 5, -1, None, None, float(EPS), strict, out.data_ptr(),
                        cnt.data_ptr(), None, None, None, None, stream())
    assert cnt.tolist() == [int(mask.sum()), -9]
    assert_rows(out, raw[mask, :5])


# ---- sps_submap_voxel and sps_filter_prepare: k_keep_count / k_keep_write<ROWS5> ---------------------------------------
DS = 0.5


@pytest.fixture
def own_map():
    yield
    util._MAP_CACHE.clear()             # the context's map is this test's now: util.prune uploads its own again


def voxel_scan(n, mask):
    """n distinct voxels (>= 1 on every axis, so truncation and floor agree), a point in the middle of each; the map
    holds the selected ones in another order"""
    i = np.arange(n)
    v = np.c_[1 + i % 61, 1 + (i // 61) % 7, 1 + i // 427].astype(np.float32)
    scan = ((v + np.float32(0.5)) * np.float32(DS)).astype(np.float32)  # exact in float32, and so is scan / DS
    mp = scan[mask][np.random.default_rng(5).permutation(int(mask.sum()))]
    dm, dscan = dev(mp), dev(scan)
    ctx().map_upload(dm.data_ptr() if len(mp) else None, 3, len(mp), DS, stream())
    torch.cuda.current_stream().synchronize()                          # the map's rows are read before dm goes
    return dscan, scan, (v[mask] * np.float32(DS)).astype(np.float32)


@cases
def test_submap_voxel(n, pattern, own_map):
    mask = keep_mask(pattern, n)
    dscan, _, want = voxel_scan(n, mask)
    out = canary(n + 2, 3)
    assert ctx().submap_voxel(dscan.data_ptr(), 3, n, out.data_ptr(), stream()) == (int(mask.sum()), n)
    assert_rows(out, want)


@cases
def test_filter_prepare(n, pattern, own_map):
    mask = keep_mask(pattern, n)
    dscan, scan, want = voxel_scan(n, mask)
    k = int(mask.sum())
    batch, counts = canary(2 * n + 2, 5), torch.full((4,), -9, dtype=torch.int32, device="cuda")
    ctx().filter_prepare(dscan.data_ptr(), False, 3, n, None, batch.data_ptr(), counts.data_ptr(), stream())
    ctx().check_errors(stream())
    assert counts.tolist() == [k, n, n + k, -9]
    np.testing.assert_array_equal(bits(batch[:n]), bits(np.c_[np.zeros(n), scan, np.ones(n)].astype(np.float32).reshape(-1, 5)))
    assert_rows(batch[n:], np.c_[np.zeros(k), want, np.zeros(k)].astype(np.float32).reshape(-1, 5))
