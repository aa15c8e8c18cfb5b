"""GPU tests of distribution-to-distribution NDT (sps_ndt_source_build, sps_ndt_align_d2d, NDTLocaliser(source="cells");
C ABI: the "NDT localiser, distribution to distribution" section of include/sps_hip.h) against the numpy restatement in
tests/ndt_d2d_reference.py.  The scene is that of test_hip_ndt.py: 400 x 32 rays, the 57 k-point synthetic map, a
12.8 k-point scan thinned at leaf 0.2 (8 160 points, 483 valid source cells) and 0.4 (4 157 points, 246)."""
import math

import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_d2d_reference as DR
from tests import ndt_reference as NR
from tests.helpers import CFG, net_from_params
from tests.test_ndt_d2d_cpu import EIG_RATIO, KW, T_INIT, T_TRUE, first_valid, sensor_scan, zero_cov_comparison

pytestmark = pytest.mark.gpu

RES = 1.0
TOL_FLOOR = 1e-12
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def map_xyz():
    return synthetic.build_map(**KW)[:, :3].astype(np.float64)


@pytest.fixture(scope="module")
def cmap(map_xyz):
    return NR.cells(map_xyz, RES)


@pytest.fixture(scope="module")
def locs(map_xyz):
    from sps_amd.localiser import NDTLocaliser
    return {leaf: NDTLocaliser(map_xyz, resolution=RES, leaf=leaf, source="cells") for leaf in (0.2, 0.4)}


@pytest.fixture(scope="module")
def scene(cmap):
    """scan 1, its thinned points and source cells at both leaves, the restatement's alignments (forward and reversed)
    and the pose tolerances that follow from their spread (read-only)"""
    scan = sensor_scan(1)
    out = dict(scan=scan)
    for leaf in (0.2, 0.4):
        pts = LR.downsample(scan, len(scan), leaf)[1]
        src = DR.sources(pts, RES, 6, EIG_RATIO)
        fwd, rev = DR.align(src, cmap, T_INIT), DR.align(src, cmap, T_INIT, reverse=True)
        st, sr = LR.pose_difference(fwd["pose"], rev["pose"])
        print(f"leaf {leaf}: spread forward/reversed {st:.3e} m {sr:.3e} rad")
        out[leaf] = dict(pts=pts, src=src, fwd=fwd, rev=rev, tol_t=max(100.0 * st, TOL_FLOOR), tol_r=max(100.0 * sr, TOL_FLOOR))
    return out


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_build(loc, pts, n=None, cap=None, res=RES, min_points=6, eig_ratio=EIG_RATIO, scratch=None):
    """sps_ndt_source_build itself on float64 points: (records [cap, 10], counts [cap], n_src), the rows pre-filled"""
    from sps_amd import _native
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    cap = len(pts) if cap is None else cap
    buf = np.zeros((max(cap, len(pts), 1), 3))
    buf[:len(pts)] = pts
    p = dev(buf)
    n_dev = torch.tensor([len(pts) if n is None else n], dtype=torch.int32, device="cuda")
    src = torch.full((max(cap, 1), 10), SENTINEL, dtype=torch.float64, device="cuda")
    cnt = torch.full((max(cap, 1),), -7, dtype=torch.int32, device="cuda")
    n_src = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    if scratch is None:
        scratch = torch.empty(_native.lib.sps_ndt_source_scratch(cap), dtype=torch.uint8, device="cuda")
    loc.ctx.ndt_source_build(p.data_ptr(), n_dev.data_ptr(), cap, res, min_points, eig_ratio, src.data_ptr(), cnt.data_ptr(),
                             n_src.data_ptr(), scratch.data_ptr(), stream())
    out = src.cpu().numpy(), cnt.cpu().numpy(), tuple(int(v) for v in n_src.cpu().numpy())
    loc.ctx.check_errors(stream())
    return out


def assert_build_is(got, want, what=""):
    rec, cnt, n_src = got
    C = want["n_src"][0]
    assert n_src == want["n_src"], what
    assert rec[:C].tobytes() == DR.records(want).tobytes(), what
    np.testing.assert_array_equal(cnt[:C], want["count"], what)
    assert (rec[C:] == SENTINEL).all() and (cnt[C:] == -7).all(), what    # rows past the cells are untouched


def raw_align(loc, rec, n_src=None, cap=None, T=T_INIT, iters=30, neighbours=7, min_corr=50, outlier_ratio=0.55):
    """sps_ndt_align_d2d itself on hand-uploaded records: dict(pose, status, iterations, n_corr, trace, normal)"""
    from sps_amd import _native
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, 10)
    cap = len(rec) if cap is None else cap
    r = dev(np.concatenate([rec, np.zeros((1, 10))]))
    n = torch.tensor([len(rec) if n_src is None else n_src, 0], dtype=torch.int32, device="cuda")
    out = torch.zeros(16 + 2 + 32 * max(iters, 1), dtype=torch.float64, device="cuda")
    scratch = torch.empty(_native.lib.sps_ndt_align_d2d_scratch(cap), dtype=torch.uint8, device="cuda")
    base = out.data_ptr()
    loc.ctx.ndt_align_d2d(r.data_ptr(), n.data_ptr(), cap, T, iters, neighbours, min_corr, outlier_ratio, 1e-4, 1e-5, base,
                          base + 16 * 8, base + 18 * 8 if iters else None, base + (18 + 4 * iters) * 8 if iters else None,
                          scratch.data_ptr(), stream())
    h = out.cpu().numpy()
    loc.ctx.check_errors(stream())
    code, it, n_corr, _ = (int(x) for x in h[16:18].view(np.int32))
    return dict(pose=h[:16].reshape(4, 4).copy(), status=code, iterations=it, n_corr=n_corr,
                trace=h[18:18 + 4 * iters].reshape(iters, 4)[:it], normal=h[18 + 4 * iters:18 + 32 * iters].reshape(iters, 28)[:it])


# ---- 1. the source build -------------------------------------------------------------------------------------------------
def one_cell_each(n):
    """n points, each in a cell of its own, in a shuffled order"""
    c = np.stack(np.unravel_index(np.random.default_rng(n).permutation(12 ** 3)[:n], (12, 12, 12)), axis=1).astype(np.float64)
    return c - 6.0 + 0.1 + 0.8 * np.random.default_rng(n + 1).random((n, 3))


def few_cells(n):
    """n points over the 40 cells of [-2, 2) x [-2, 3) x [0, 2)"""
    return np.random.default_rng(n).random((n, 3)) * [4.0, 5.0, 2.0] - [2.0, 2.0, 0.0]


def test_source_build_hand_built_cells(locs):
    hb, names = DR.hand_built_points()
    want = DR.sources(hb, RES, 6, EIG_RATIO)
    got = raw_build(locs[0.4], hb, cap=len(hb) + 5)
    assert_build_is(got, want)
    row = {k: DR.find_source(want, v) for k, v in names.items()}
    valid = got[0][:6, 9] != 0.0
    assert [bool(valid[row[k]]) for k in ("five", "six", "same", "plane", "neg", "face")] == [False, True, False, True, False, False]


@pytest.mark.parametrize("n", [0, 1])
def test_source_build_of_nothing_and_of_one_point(locs, n):
    pts = np.array([[0.25, -0.5, 1.75]])[:n]
    assert_build_is(raw_build(locs[0.4], pts, cap=4), DR.sources(pts, RES, 6, EIG_RATIO))
    assert_build_is(raw_build(locs[0.4], pts, cap=n), DR.sources(pts, RES, 6, EIG_RATIO), "cap = n")


def test_source_build_all_points_in_one_cell(locs):
    pts = 3.0 + 0.05 + 0.9 * np.random.default_rng(2).random((700, 3))    # 700 points: eleven chunks of the wave's loop
    want = DR.sources(pts, RES, 6, EIG_RATIO)
    assert want["n_src"] == (1, 1) and want["count"][0] == 700
    assert_build_is(raw_build(locs[0.4], pts), want)


@pytest.mark.parametrize("n", [31, 32, 33, 1023, 1024, 1025])
def test_source_build_every_point_its_own_cell(locs, n):
    pts = one_cell_each(n)
    want = DR.sources(pts, RES, 1, EIG_RATIO)
    assert want["n_src"] == (n, 0)                                        # one point: no covariance, never valid
    assert_build_is(raw_build(locs[0.4], pts, min_points=1), want)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_source_build_over_about_forty_cells(locs, n):
    pts = few_cells(n)
    want = DR.sources(pts, RES, 6, EIG_RATIO)
    assert 35 <= want["n_src"][0] <= 40 and want["n_src"][1] >= 10
    assert_build_is(raw_build(locs[0.4], pts), want)
    want = DR.sources(pts, 0.5, 3, 0.1)                                   # another resolution, min_points and eig_ratio
    assert_build_is(raw_build(locs[0.4], pts, res=0.5, min_points=3, eig_ratio=0.1), want, "0.5 m")


def test_source_build_reads_only_cap_points_and_skips_bad_rows(locs):
    pts = few_cells(300)
    assert_build_is(raw_build(locs[0.4], pts, n=300, cap=200), DR.sources(pts[:200], RES, 6, EIG_RATIO), "n_dev > cap")
    assert_build_is(raw_build(locs[0.4], pts, n=-3), DR.sources(pts[:0], RES, 6, EIG_RATIO), "n_dev < 0")
    bad = pts.copy()
    bad[3, 0], bad[50, 1], bad[120, 2], bad[121, 0] = np.nan, 1048576.5, -np.inf, -1048576.5
    edge = np.array([[1048575.5, 0.5, 0.5], [-1048574.5, 0.5, 0.5]])       # the last cells of the key range are kept
    bad = np.concatenate([bad, edge])
    want = DR.sources(bad, RES, 6, EIG_RATIO)
    clean = DR.sources(np.delete(bad, [3, 50, 120, 121], axis=0), RES, 6, EIG_RATIO)
    assert DR.records(want).tobytes() == DR.records(clean).tobytes()      # skipped rows leave no trace
    assert_build_is(raw_build(locs[0.4], bad), want, "bad rows")


@pytest.mark.parametrize("leaf", [0.2, 0.4])
def test_source_cells_of_the_scene_twice(locs, scene, leaf):
    want = scene[leaf]["src"]
    scan = dev(scene["scan"])
    a = locs[leaf].source_cells(scan, len(scan))
    b = locs[leaf].source_cells(scan, len(scan))
    for k in ("mean", "cov", "count", "valid"):
        assert a[k].tobytes() == b[k].tobytes(), k                        # two calls, the same bits
    np.testing.assert_array_equal(a["count"], want["count"])
    np.testing.assert_array_equal(a["valid"], want["valid"])
    assert a["mean"].tobytes() == want["mean"].tobytes() and a["cov"].tobytes() == want["cov"].tobytes()
    assert_build_is(raw_build(locs[leaf], scene[leaf]["pts"], cap=len(scene[leaf]["pts"]) + 7), want, "raw")


# ---- 2. one iteration, term by term --------------------------------------------------------------------------------------
def check_one_iteration(loc, cmap, src, min_corr=1):
    """Bound of every normal-equation entry against math.fsum of the restatement's per-pair terms: (m + 6) * 2^-52 * sum |t|,
    as tests/test_hip_ndt.py derives it (m addends in any fixed order, and the two exp libraries within their documented
    error), m = the contributing pairs."""
    ref = DR.align(src, cmap, T_INIT, iters=1, min_corr=min_corr)
    assert ref["faces"] == 0 and ref["boundary"] == 0                      # exact counts need neither
    got = raw_align(loc, DR.records(src), iters=1, min_corr=min_corr)
    assert (got["status"], got["iterations"]) == (ref["status"], 1) and ref["status"] == 1
    assert got["n_corr"] == ref["n_corr"] == int(got["trace"][0, 0])
    terms = ref["terms"][0]
    m = len(terms)
    assert m >= ref["n_corr"] > 0
    worst = 0.0
    for k in range(28):
        sum_abs = math.fsum(np.abs(terms[:, k]))
        bound = (m + 6) * 2.0 ** -52 * sum_abs
        exact = math.fsum(terms[:, k])
        worst = max(worst, abs(got["normal"][0, k] - exact) / max(bound, 1e-300))
        assert abs(got["normal"][0, k] - exact) <= bound, k
    print(f"{ref['n_corr']} sources, {m} pairs: worst |device - fsum| / bound {worst:.3f}")
    assert got["trace"][0, 1] == got["normal"][0, 27]
    return ref


@pytest.mark.parametrize("k", [31, 32, 33, 65])
def test_one_iteration_at_k_valid_sources(locs, cmap, scene, k):
    src = scene[0.4]["src"]
    sub = first_valid(src, k)
    assert sub["n_src"][1] == k and sub["n_src"][0] > k                    # invalid records in between keep their slots
    ref = check_one_iteration(locs[0.4], cmap, sub)
    assert ref["n_corr"] <= k


@pytest.mark.parametrize("leaf", [0.2, 0.4])
def test_one_iteration_on_the_scene(locs, cmap, scene, leaf):
    ref = check_one_iteration(locs[leaf], cmap, scene[leaf]["src"], min_corr=50)
    assert ref["n_corr"] > 200
    q = LR.transform(scene[leaf]["src"]["mean"], T_INIT)
    assert (q.min(axis=0) < 0).all()                                       # negative map coordinates on every axis
    res = locs[leaf](dev(scene["scan"]), len(scene["scan"]), T_INIT, with_normal=True, iterations=1)
    raw = raw_align(locs[leaf], DR.records(scene[leaf]["src"]), iters=1)
    assert res.normal.tobytes() == raw["normal"].tobytes()                 # the localiser issues exactly these two calls
    assert (res.n_points, res.n_sources, res.n_corr) == (len(scene[leaf]["pts"]), scene[leaf]["src"]["n_src"][1], ref["n_corr"])


# ---- 3. the full alignment -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [0.2, 0.4])
def test_full_alignment_matches_the_restatement(locs, scene, leaf):
    s = scene[leaf]
    fwd = s["fwd"]
    res = locs[leaf](dev(scene["scan"]), len(scene["scan"]), T_INIT)
    assert fwd["status"] == 0 and fwd["faces"] == 0 and fwd["boundary"] == 0
    assert (res.status, res.iterations) == (fwd["status"], fwd["iterations"])
    np.testing.assert_array_equal(res.trace[:, 0], fwd["trace"][:, 0])     # the sources counted in every iteration
    dt, dr = LR.pose_difference(res.pose, fwd["pose"])
    et, er = LR.pose_difference(res.pose, T_TRUE)
    print(f"leaf {leaf}: {res.iterations} iterations, {res.n_corr} of {res.n_sources} sources; device vs restatement {dt:.3e} m "
          f"{dr:.3e} rad (tolerance {s['tol_t']:.3e} m {s['tol_r']:.3e} rad); error against the truth {et * 1e3:.2f} mm")
    assert dt <= s["tol_t"] and dr <= s["tol_r"]
    again = locs[leaf](dev(scene["scan"]), len(scene["scan"]), T_INIT)
    assert again.pose.tobytes() == res.pose.tobytes() and again.trace.tobytes() == res.trace.tobytes()


# ---- 4. zero-covariance sources ------------------------------------------------------------------------------------------
def test_zero_covariance_sources_follow_the_point_alignment(map_xyz, locs, cmap, scene):
    """Hand-uploaded sources with C = 0 at the thinned points against sps_ndt_align on those points: the same status and
    iteration count, the pose within 100 x the difference the restatements of the two paths show between themselves on the
    CPU (floored at 1e-12)."""
    from sps_amd.localiser import NDTLocaliser
    pts = scene[0.4]["pts"]
    p2d = NR.align(pts, cmap, T_INIT)
    d2d = DR.align(DR.hand_sources(pts), cmap, T_INIT)
    assert (p2d["status"], p2d["iterations"]) == (d2d["status"], d2d["iterations"]) and p2d["status"] == 0
    st, sr = LR.pose_difference(p2d["pose"], d2d["pose"])
    tol_t, tol_r = max(100.0 * st, TOL_FLOOR), max(100.0 * sr, TOL_FLOOR)
    points = NDTLocaliser(map_xyz, resolution=RES, leaf=0.4)
    a = points(dev(scene["scan"]), len(scene["scan"]), T_INIT)
    b = raw_align(locs[0.4], DR.records(DR.hand_sources(pts)))
    dt, dr = LR.pose_difference(a.pose, b["pose"])
    print(f"restatements differ by {st:.3e} m {sr:.3e} rad -> tolerance {tol_t:.3e} m {tol_r:.3e} rad; devices {dt:.3e} m {dr:.3e} rad")
    assert (a.status, a.iterations) == (b["status"], b["iterations"]) == (p2d["status"], p2d["iterations"])
    np.testing.assert_array_equal(a.trace[:, 0], b["trace"][:, 0])
    assert dt <= tol_t and dr <= tol_r
    # the score: its terms within the CPU test's 16 * 2^-52 / eig_ratio, and the poses it is taken at within the tolerance
    # above (the score changes by less than 100 x itself per metre or radian here: |g| / score < 10 in the CPU test's print)
    np.testing.assert_allclose(b["trace"][:, 1], a.trace[:, 1], rtol=16 * 2.0 ** -52 / EIG_RATIO + 100 * (tol_t + tol_r))
    hp, hd, _ = zero_cov_comparison(cmap, pts, T_INIT)                     # the CPU test's input, on the device side too
    assert len(hp["i"]) == len(hd["i"])


# ---- 5. edges --------------------------------------------------------------------------------------------------------------
def test_edges(locs, cmap, scene):
    from sps_amd.localiser import NDTLocaliser
    src = scene[0.4]["src"]
    rec = DR.records(src)
    loc = locs[0.4]
    T0 = np.asarray(T_INIT, dtype=np.float64)
    empty = NDTLocaliser(np.zeros((0, 3)), resolution=RES, leaf=0.4, source="cells")
    r = empty(dev(scene["scan"]), len(scene["scan"]), T_INIT)
    assert (r.status, r.iterations, r.n_corr) == (2, 1, 0) and r.pose.tobytes() == T0.tobytes()
    assert r.n_sources == src["n_src"][1] and r.n_points == len(scene[0.4]["pts"])
    invalid = rec.copy()
    invalid[:, 9] = 0.0
    r = raw_align(loc, invalid)
    assert (r["status"], r["iterations"], r["n_corr"]) == (2, 1, 0) and r["pose"].tobytes() == T0.tobytes()
    r = raw_align(loc, rec, iters=0)
    assert (r["status"], r["iterations"]) == (1, 0) and r["pose"].tobytes() == T0.tobytes()
    r = raw_align(loc, rec[:0], cap=0)                                     # no records at all
    assert r["status"] == 2 and r["pose"].tobytes() == T0.tobytes()
    one = DR.align(src, cmap, T_INIT, iters=1)
    r = raw_align(loc, rec, min_corr=one["n_corr"] + 1)
    assert (r["status"], r["iterations"], r["n_corr"]) == (2, 1, one["n_corr"]) and r["pose"].tobytes() == T0.tobytes()
    r = raw_align(loc, rec, min_corr=one["n_corr"], iters=1)
    assert r["status"] == 1
    r = raw_align(loc, rec, n_src=len(rec) + 99, iters=1)                  # a count beyond cap_src is clamped
    assert r["n_corr"] == one["n_corr"]
    # a source whose neighbourhood leaves the key range, and one beyond it: neither contributes, the rest is as before
    far = np.zeros((2, 10))
    far[0, :3], far[1, :3] = [1048575.5, 0.5, 0.5], [3.0e6, 0.5, 0.5]
    far[:, [3, 6, 8]], far[:, 9] = 0.01, 1.0
    a = raw_align(loc, np.concatenate([rec, far]), T=np.eye(4), iters=1, min_corr=1)
    b = raw_align(loc, rec, T=np.eye(4), iters=1, min_corr=1)
    ref = DR.align(DR.hand_sources(np.concatenate([rec, far])[:, :3], np.concatenate([rec, far])[:, 3:9],
                                   np.concatenate([rec, far])[:, 9] != 0.0), cmap, np.eye(4), iters=1, min_corr=1)
    assert a["n_corr"] == b["n_corr"] == ref["n_corr"] and a["normal"].tobytes() == b["normal"].tobytes()
    for bad in (dict(neighbours=3), dict(outlier_ratio=1.5), dict(iters=10001)):
        with pytest.raises(Exception):
            raw_align(loc, rec, **bad)
    loc.ctx.check_errors(stream())


def test_an_online_map_after_one_integrate(map_xyz, scene):
    from sps_amd.localiser import NDTLocaliser
    dyn = NDTLocaliser(map_xyz, resolution=RES, leaf=0.4, source="cells", cell_capacity=8192)
    scan2 = sensor_scan(2)
    u = dyn.integrate(dev(scan2), len(scan2), T_TRUE).result()
    assert u.points > 1000
    key, count, mean, icov, valid = dyn.map_cells()
    order = np.argsort(key)                                                # the restatement looks cells up by ascending key
    m = dict(keys=key[order], count=count[order].astype(np.int64), mean=mean[order], icov=icov[order], valid=valid[order],
             resolution=RES)
    src = scene[0.4]["src"]
    fwd, rev = DR.align(src, m, T_INIT), DR.align(src, m, T_INIT, reverse=True)
    st, sr = LR.pose_difference(fwd["pose"], rev["pose"])
    res = dyn(dev(scene["scan"]), len(scene["scan"]), T_INIT)
    assert (res.status, res.iterations) == (fwd["status"], fwd["iterations"]) and fwd["faces"] == 0 and fwd["boundary"] == 0
    np.testing.assert_array_equal(res.trace[:, 0], fwd["trace"][:, 0])
    dt, dr = LR.pose_difference(res.pose, fwd["pose"])
    assert dt <= max(100.0 * st, TOL_FLOOR) and dr <= max(100.0 * sr, TOL_FLOOR)
    dyn.ctx.check_errors(stream())


# ---- 6. stream order and the loop ----------------------------------------------------------------------------------------
def test_integrate_and_carve_behind_a_d2d_alignment_on_a_side_stream(map_xyz, scene):
    """submit(integrate=True, carve=True) with source="cells" on a side stream leaves the map, the update's and the carve's
    results that the point path's carve and integrate leave when they are fed the pose the D2D alignment found."""
    from sps_amd.localiser import NDTLocaliser
    opts = dict(min_pass=1, miss_frames=1, through_sigma=2.0)
    cells = NDTLocaliser(map_xyz, resolution=RES, leaf=0.4, source="cells", cell_capacity=8192)
    points = NDTLocaliser(map_xyz, resolution=RES, leaf=0.4, cell_capacity=8192)
    scan = dev(scene["scan"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pend = cells.submit(scan, len(scan), T_INIT, integrate=True, carve=True, carve_options=opts)
    r = pend.result()
    assert r.status == 0 and r.iterations == scene[0.4]["fwd"]["iterations"] and r.n_sources == scene[0.4]["src"]["n_src"][1]
    c = points.carve(scan, len(scan), r.pose, **opts).result()
    u = points.integrate(scan, len(scan), r.pose).result()
    assert [r.map_carve.rays, r.map_carve.seen_through, r.map_carve.cleared, r.map_carve.cut] == [c.rays, c.seen_through, c.cleared, c.cut]
    assert [r.map_update.cells, r.map_update.founded, r.map_update.dropped, r.map_update.points] == [u.cells, u.founded, u.dropped, u.points]
    assert u.points > 1000 and c.rays > 1000
    for a, b in zip(cells.map_cells(), points.map_cells()):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(cells.carve_state(), points.carve_state()):
        assert a.tobytes() == b.tobytes()
    cells.ctx.check_errors(stream())


class RestatementD2D:
    """tests/ndt_d2d_reference.py behind the interface LocalisationLoop uses"""

    def __init__(self, cmap, like):
        self.cmap, self.like, self.device = cmap, like, like.device

    def submit_filtered(self, pending, T_init):
        from sps_amd.localiser import PoseResult
        n = int(pending.count_dev.item())
        rows = pending._filtered[:n].cpu().numpy()
        L = self.like
        _, pts = LR.downsample(rows, n, L.leaf, L.capacity)
        src = DR.sources(pts, L.source_resolution, L.source_min_points, L.eig_ratio)
        r = DR.align(src, self.cmap, T_init, L.iterations, L.neighbours, L.min_correspondences, L.outlier_ratio, L.tol_t, L.tol_r)
        assert r["faces"] == 0 and r["boundary"] == 0
        res = PoseResult(r["pose"], r["status"], r["iterations"], r["n_corr"], float("nan"), r["trace"], None, len(pts),
                         n_sources=src["n_src"][1])

        class Done:
            def result(self):
                return res
        return Done()


def test_three_loop_frames_follow_the_restatement(scene):
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser
    from sps_amd.sps_filters import SPSCVMFilter
    n, step = 3, 0.5
    mp = synthetic.sequence_map(n, step, **KW)
    truth, scans = [], []
    for i in range(n):
        world = synthetic.lidar_scan(100 + i, x_offset=step * i, **KW)
        T = LR.perturbation(step * i, 0.0, 0.0, math.degrees(0.02 * i))
        Ti = np.linalg.inv(T)
        scans.append(np.c_[world[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3], world[:, 3]].astype(np.float32))
        truth.append(T)
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(np.ascontiguousarray(mp[:, :3], dtype=np.float32))
    map64 = mp[:, :3].astype(np.float64)

    def run(localiser):
        loop = LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0), localiser, truth[0])
        steps = [loop.step(s) for s in scans]
        return loop.poses, steps

    ndt = NDTLocaliser(map64, resolution=RES, leaf=0.4, source="cells")
    got, steps = run(ndt)
    want, ref_steps = run(RestatementD2D(NR.cells(map64, RES), ndt))
    for i in range(n):
        a, b = steps[i].pose_result, ref_steps[i].pose_result
        dt, dr = LR.pose_difference(got[i], want[i])
        print(f"frame {i}: status {a.status}/{b.status} iterations {a.iterations}/{b.iterations} sources {a.n_corr}/{b.n_corr} of "
              f"{a.n_sources}/{b.n_sources}; device vs restatement {dt:.3e} m {dr:.3e} rad")
        assert (a.status, a.iterations, a.n_corr, a.n_points, a.n_sources) == (b.status, b.iterations, b.n_corr, b.n_points, b.n_sources), i
        assert dt <= scene[0.4]["tol_t"] and dr <= scene[0.4]["tol_r"], i
    with pytest.raises(ValueError):
        LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0), ndt, truth[0],
                         hypotheses=np.eye(4)[None])
    ndt.ctx.check_errors(stream())
    # with an online map, the carve and an estimator: the loop fetches the predicted pose first (submit_from_device is
    # point-only) and every frame reports its update and its carve
    from sps_amd.pose_estimator import PoseEstimator
    n_cells = ndt.n_cells
    dyn = NDTLocaliser(map64, resolution=RES, leaf=0.4, source="cells", cell_capacity=2 * n_cells)
    make = lambda: SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0)
    with pytest.raises(ValueError):
        LocalisationLoop(make(), dyn, truth[0], estimator=PoseEstimator(truth[0], dyn.device), device_guess=True)
    est = PoseEstimator(truth[0], dyn.device, initial_velocity=(step / 0.1, 0.0, 0.0))
    loop = LocalisationLoop(make(), dyn, truth[0], update_map=True, carve_map=True, estimator=est)
    assert loop.device_guess is False
    for i, s in enumerate(scans):
        st = loop.step(s, dt=0.1)
        p = st.pose_result
        assert not st.flagged and p.status in (0, 1) and p.n_sources >= p.n_corr >= dyn.min_correspondences, i
        assert p.map_update.points > 1000 and p.map_carve.rays > 1000 and st.estimate is not None, i
    dyn.ctx.check_errors(stream())


def test_source_points_gives_the_bits_of_a_localiser_without_the_argument(map_xyz, scene):
    from sps_amd.localiser import NDTLocaliser
    a = NDTLocaliser(map_xyz, resolution=RES, leaf=0.4, source="points")
    b = NDTLocaliser(map_xyz, resolution=RES, leaf=0.4)
    scan = dev(scene["scan"])
    ra, rb = a(scan, len(scan), T_INIT, with_normal=True), b(scan, len(scan), T_INIT, with_normal=True)
    assert (ra.status, ra.iterations, ra.n_corr, ra.n_points, ra.n_sources) == (rb.status, rb.iterations, rb.n_corr, rb.n_points, 0)
    assert ra.pose.tobytes() == rb.pose.tobytes() and ra.trace.tobytes() == rb.trace.tobytes()
    assert ra.normal.tobytes() == rb.normal.tobytes() and ra.iterations > 1
    for ma, mb in zip(a.map_cells(), b.map_cells()):
        assert ma.tobytes() == mb.tobytes()


def test_refusals_on_a_device_localiser(locs, scene):
    loc = locs[0.4]
    scan = dev(scene["scan"])
    poses = np.eye(4)[None]
    for call in (lambda: loc.submit_batch(scan, len(scan), poses), lambda: loc.score_poses(scan, len(scan), poses),
                 lambda: loc.relocalise(scan, len(scan), poses),
                 lambda: loc.submit_from_device(scan, len(scan), dev(np.eye(4).reshape(16)))):
        with pytest.raises(ValueError, match="source='points'"):
            call()
