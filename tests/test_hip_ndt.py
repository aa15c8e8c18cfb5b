"""GPU tests of the NDT localiser (sps_amd.localiser.NDTLocaliser; C ABI: the "NDT localiser" section of
include/sps_hip.h) against the numpy restatement in tests/ndt_reference.py.  Shapes are those of test_hip_localiser.py:
400 x 32 rays, the 57 k-point synthetic map, a 12.8 k-point scan thinned at leaf 0.4 to ~4.2 k points."""
import math

import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_reference as NR
from tests.helpers import CFG, net_from_params, straddle_params
from tests.test_ndt_cpu import KW, LEAF, T_INIT, T_TRUE, sensor_scan

pytestmark = pytest.mark.gpu

RES = 1.0
# this project's rule for float64 comparisons that differ only in the order of a sum (test_hip_localiser.py)
TOL_FLOOR = 1e-12


@pytest.fixture(scope="module")
def map_xyz():
    """the synthetic map plus the hand-built cells of test_ndt_cpu.py (invalid, identical, coplanar, x < 0)"""
    hb, _ = NR.hand_built_cells()
    return np.concatenate([synthetic.build_map(**KW)[:, :3].astype(np.float64), hb])


@pytest.fixture(scope="module")
def cmap(map_xyz):
    return NR.cells(map_xyz, RES)


@pytest.fixture(scope="module")
def loc(map_xyz):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(map_xyz, resolution=RES, leaf=LEAF)


@pytest.fixture(scope="module")
def loc1(map_xyz):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(map_xyz, resolution=RES, leaf=LEAF, neighbours=1)


@pytest.fixture(scope="module")
def full(cmap):
    """the restatement's full alignment of scan 1, forward and reversed, and the pose tolerance that follows from it"""
    scan = sensor_scan(1)
    _, pts = LR.downsample(scan, len(scan), LEAF)
    fwd = NR.align(pts, cmap, T_INIT)
    rev = NR.align(pts, cmap, T_INIT, reverse=True)
    spread_t, spread_r = LR.pose_difference(fwd["pose"], rev["pose"])
    tol_t, tol_r = max(100.0 * spread_t, TOL_FLOOR), max(100.0 * spread_r, TOL_FLOOR)
    print(f"spread forward/reversed: {spread_t:.3e} m {spread_r:.3e} rad -> tolerance {tol_t:.3e} m {tol_r:.3e} rad")
    return dict(scan=scan, pts=pts, fwd=fwd, rev=rev, tol_t=tol_t, tol_r=tol_r)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    assert (a.status, a.iterations, a.n_corr, a.n_points) == (b.status, b.iterations, b.n_corr, b.n_points)
    for x, y in ((a.pose, b.pose), (a.trace, b.trace), (a.normal, b.normal)):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()


# ---- the map ---------------------------------------------------------------------------------------------------------------
def test_map_cells_match_the_restatement(loc, cmap, map_xyz):
    key, count, mean, icov, valid = loc.map_cells()
    np.testing.assert_array_equal(key, cmap["keys"])
    np.testing.assert_array_equal(count, cmap["count"])
    np.testing.assert_array_equal(valid, cmap["valid"])
    assert 1000 < valid.sum() < len(valid)
    # the hand-built cells took the branches they were built for, on the device
    _, names = NR.hand_built_cells()
    row = {k: NR.find_cell(cmap, v) for k, v in names.items()}
    assert not valid[row["five"]] and valid[row["six"]] and not valid[row["same"]] and valid[row["plane"]] and not valid[row["neg"]]
    assert (count[[row["five"], row["six"], row["same"], row["plane"], row["neg"]]] == [5, 6, 6, 6, 1]).all()
    # tolerance: 100 x the spread between the restatement's Jacobi route and its numpy.linalg.eigh route on the same
    # cells, relative to the Frobenius norm of the inverse covariance, floored at 1e-12
    eigh = NR.cells(map_xyz, RES, route="eigh")
    v = cmap["valid"]

    def frob(m6):
        return np.sqrt((m6 ** 2).sum(axis=1) + (m6[:, [1, 2, 4]] ** 2).sum(axis=1))
    nrm = frob(cmap["icov"][v])
    spread = float((frob(cmap["icov"][v] - eigh["icov"][v]) / nrm).max())
    tol = max(100.0 * spread, TOL_FLOOR)
    got = float((frob(icov[v] - cmap["icov"][v]) / nrm).max())
    got_mean = float(np.abs(mean - cmap["mean"]).max() / np.abs(cmap["mean"]).max())
    print(f"icov: Jacobi/eigh spread {spread:.3e} -> tolerance {tol:.3e}; device vs restatement {got:.3e}; mean {got_mean:.3e}")
    assert got <= tol and got_mean <= tol
    p = row["plane"]                                                       # the floored direction: 1 / (0.01 lambda_max)
    assert icov[p][5] == pytest.approx(1.0 / cmap["lam"][p].min(), rel=tol)


# ---- one iteration ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("neighbours", [7, 1])
def test_one_iteration_matches_the_restatement(loc, loc1, cmap, full, neighbours):
    """Bound of every normal-equation entry against math.fsum of the restatement's per-cell terms t_1 .. t_m:
      * summing m addends in any fixed order rounds at most m - 1 times, each time by <= 2^-53 of a partial sum that
        is <= sum |t|: m * 2^-52 * sum |t| covers it with a factor 2 to spare (the bound of test_hip_localiser.py);
      * a device term differs from the restatement's only through exp: the argument has the same bits on both sides,
        HIP documents exp(double) as good to 1 ulp, the C library behind numpy likewise, so the two values of e differ
        by <= 2 ulp <= 2 * 2^-52 relative; w = d2 * e, a = -d1 * w and term = a * h then round three times on either
        side, 6 * 2^-53 = 3 * 2^-52 more.  5 * 2^-52 in all; 6 * 2^-52 * sum |t| is used.
    Together (m + 6) * 2^-52 * sum |t|."""
    L = loc if neighbours == 7 else loc1
    scan, pts = full["scan"], full["pts"]
    ref = NR.align(pts, cmap, T_INIT, iters=1, neighbours=neighbours)
    # exact counts need an input without a point on a cell face and without a weight on the guard's boundary
    assert ref["faces"] == 0 and ref["boundary"] == 0
    q = LR.transform(pts, T_INIT)
    assert (q.min(axis=0) < 0).all()                                       # negative map coordinates on every axis
    res = L(dev(scan), len(scan), T_INIT, with_normal=True, iterations=1)
    assert res.n_points == len(pts)
    assert res.iterations == 1 and res.status == 1 and ref["status"] == 1
    assert res.n_corr == ref["n_corr"] and int(res.trace[0, 0]) == ref["n_corr"] and ref["n_corr"] > 1000
    terms = ref["terms"][0]
    m = len(terms)
    assert m > ref["n_corr"] or neighbours == 1
    for k in range(28):
        sum_abs = math.fsum(np.abs(terms[:, k]))
        bound = (m + 6) * 2.0 ** -52 * sum_abs
        exact = math.fsum(terms[:, k])
        print(f"normal[{k}]: device {res.normal[0, k]!r} exact {exact!r} |diff| {abs(res.normal[0, k] - exact):.3e} bound {bound:.3e}")
        assert abs(res.normal[0, k] - exact) <= bound, k
        assert abs(ref["normal"][0, k] - exact) <= m * 2.0 ** -52 * sum_abs, k
    assert res.trace[0, 1] == res.normal[0, 27]


# ---- the whole alignment ---------------------------------------------------------------------------------------------------
def test_full_alignment_matches_the_restatement(loc, full):
    fwd, tol_t, tol_r = full["fwd"], full["tol_t"], full["tol_r"]
    res = loc(dev(full["scan"]), len(full["scan"]), T_INIT)
    assert fwd["status"] == 0 and fwd["faces"] == 0 and fwd["boundary"] == 0
    assert (res.status, res.iterations) == (fwd["status"], fwd["iterations"])
    np.testing.assert_array_equal(res.trace[:, 0], fwd["trace"][:, 0])                 # the count of every iteration
    dt, dr = LR.pose_difference(res.pose, fwd["pose"])
    print(f"device vs restatement: {dt:.3e} m {dr:.3e} rad")
    assert dt <= tol_t and dr <= tol_r
    et, er = LR.pose_difference(res.pose, T_TRUE)
    rt, rr = LR.pose_difference(fwd["pose"], T_TRUE)
    print(f"error against the ground truth: device {et:.6e} m {er:.6e} rad, restatement {rt:.6e} m {rr:.6e} rad")
    assert et <= rt + tol_t and er <= rr + tol_r


def test_two_calls_give_the_same_bits(loc):
    scan = dev(sensor_scan(2))
    a = loc(scan, len(scan), T_INIT, with_normal=True)
    b = loc(scan, len(scan), T_INIT, with_normal=True)
    assert a.iterations > 1
    same_bits(a, b)


# ---- edges -----------------------------------------------------------------------------------------------------------------
def test_a_scan_off_the_map_is_an_ordinary_result(loc):
    good = dev(sensor_scan(2))
    before = loc(good, len(good), T_INIT)
    far = sensor_scan(2)
    far[:, 0] += 500.0
    res = loc(dev(far), len(far), T_INIT)
    assert res.status == 2 and res.iterations == 1 and res.n_corr < loc.min_correspondences
    assert res.pose.tobytes() == np.asarray(T_INIT, dtype=np.float64).tobytes()        # the guess, bit for bit
    loc.ctx.check_errors(stream())
    empty = loc(good, 0, T_INIT)                                                       # count = 0
    assert empty.status == 2 and empty.n_points == 0 and empty.pose.tobytes() == T_INIT.tobytes()
    none = loc(torch.zeros((0, 4), dtype=torch.float32, device="cuda"), 0, T_INIT)     # n_max = 0
    assert none.status == 2 and none.n_points == 0 and none.pose.tobytes() == T_INIT.tobytes()
    after = loc(good, len(good), T_INIT)                                               # the next call is unaffected
    assert after.status == before.status == 0
    assert after.pose.tobytes() == before.pose.tobytes() and after.trace.tobytes() == before.trace.tobytes()
    loc.ctx.check_errors(stream())


def test_bad_rows_are_skipped_and_a_large_count_is_clamped(loc):
    scan = sensor_scan(3)
    bad = [17, 400, 4000]
    rows = scan.copy()
    rows[17, 0], rows[400, 2], rows[4000, 1] = np.nan, 3.0e6, -np.inf
    clean = np.delete(scan, bad, axis=0)
    a = loc(dev(rows), len(rows), T_INIT, with_normal=True)
    b = loc(dev(clean), len(clean), T_INIT, with_normal=True)              # the survivors and their order are the same
    assert a.status in (0, 1) and a.n_corr > 1000
    same_bits(a, b)
    loc.ctx.check_errors(stream())                                         # never a sticky error
    big = torch.tensor([len(rows) + 99], dtype=torch.int32, device="cuda")
    same_bits(a, loc(dev(rows), big, T_INIT, with_normal=True))            # a count beyond n_max is clamped to it


def test_capacity_overflow_saturates(map_xyz, cmap, full):
    from sps_amd.localiser import NDTLocaliser
    cap = 1000
    small = NDTLocaliser(map_xyz, resolution=RES, leaf=LEAF, capacity=cap)
    assert len(full["pts"]) > cap
    ref = NR.align(full["pts"][:cap], cmap, T_INIT, iters=1)
    res = small(dev(full["scan"]), len(full["scan"]), T_INIT, iterations=1)
    assert res.n_points == cap and res.n_corr == ref["n_corr"] and ref["faces"] == 0
    small.ctx.check_errors(stream())


def test_an_empty_map_gives_status_2(full):
    from sps_amd.localiser import NDTLocaliser
    empty = NDTLocaliser(np.zeros((0, 3)), resolution=RES, leaf=LEAF)
    res = empty(dev(full["scan"]), len(full["scan"]), T_INIT)
    assert (res.status, res.iterations, res.n_corr) == (2, 1, 0) and res.n_points == len(full["pts"])
    assert res.pose.tobytes() == T_INIT.tobytes()
    assert len(empty.map_cells()[0]) == 0
    empty.ctx.check_errors(stream())


def test_a_scan_in_the_negative_octant(loc, cmap, full):
    q = LR.transform(full["pts"], T_INIT)
    neg = full["pts"][(q < 0).all(axis=1)]
    assert len(neg) > 200 and (LR.transform(neg, T_INIT) < 0).all()        # negative on every axis: floor, not truncation
    rows = dev(np.c_[neg, np.zeros(len(neg))].astype(np.float32))
    _, pts = LR.downsample(rows.cpu().numpy(), len(neg), LEAF)
    ref = NR.align(pts, cmap, T_INIT, iters=1, min_corr=1)
    assert ref["faces"] == 0 and ref["n_corr"] > 100
    from sps_amd.localiser import NDTLocaliser
    res = loc(rows, len(neg), T_INIT, iterations=1)
    assert res.n_points == len(pts) and res.n_corr == ref["n_corr"]
    assert isinstance(loc, NDTLocaliser)


def test_arguments_are_checked(loc, map_xyz):
    from sps_amd.localiser import NDTLocaliser
    with pytest.raises(ValueError):
        NDTLocaliser(map_xyz[:100], neighbours=27)
    with pytest.raises(ValueError):
        NDTLocaliser(map_xyz[:100], resolution=0.0)
    with pytest.raises(TypeError):
        loc.submit(torch.zeros((4, 4)), 4, T_INIT)                         # a host tensor
    with pytest.raises(ValueError):
        loc.submit(torch.zeros((4, 2), device="cuda"), 4, T_INIT)
    with pytest.raises(ValueError):
        loc.submit(torch.zeros((4, 4), device="cuda"), 5, T_INIT)


# ---- stream order: the filter's pending frame goes straight in -------------------------------------------------------------
def test_submit_filtered_equals_result_then_submit(loc, map_xyz):
    from sps_amd.sps_filters import SPSFilter
    params = straddle_params(O.random_params(seed=0), synthetic.small_scene(seed=11, n_scan=2500))
    net = net_from_params(params).cuda().eval().freeze()
    f = SPSFilter(net, map_xyz.astype(np.float32), voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=CFG["FILTER"]["THRESHOLD"])
    scan = sensor_scan(4)
    pend = f.submit(scan, T_TRUE)
    pose_pend = loc.submit_filtered(pend, T_INIT, with_normal=True)        # before the frame's result()
    a = pose_pend.result()
    fres = pend.result()
    assert 0 < len(fres.filtered) <= len(scan)
    b = loc(fres.filtered.clone(), len(fres.filtered), T_INIT, with_normal=True)
    same_bits(a, b)


# ---- the closed loop -------------------------------------------------------------------------------------------------------
class RestatementLocaliser:
    """tests/ndt_reference.py behind the interface LocalisationLoop uses"""

    def __init__(self, cmap, like):
        self.cmap, self.like, self.device = cmap, like, like.device

    def submit_filtered(self, pending, T_init):
        from sps_amd.localiser import PoseResult
        n = int(pending.count_dev.item())
        rows = pending._filtered[:n].cpu().numpy()
        L = self.like
        _, pts = LR.downsample(rows, n, L.leaf, L.capacity)
        r = NR.align(pts, self.cmap, T_init, L.iterations, L.neighbours, L.min_correspondences, L.outlier_ratio, L.tol_t, L.tol_r)
        res = PoseResult(r["pose"], r["status"], r["iterations"], r["n_corr"], float("nan"), r["trace"], None, len(pts))

        class Done:
            def result(self):
                return res
        return Done()


def test_closed_loop_follows_the_restatement(full):
    """LocalisationLoop(SPSCVMFilter, NDTLocaliser) over all 8 synthetic frames of the driver's --synthetic 8 replay (the
    numpy side takes about half a second per frame at leaf 0.4, so no restriction to 3 frames was needed).  The filter
    runs at epsilon = 2 (every point passes, the driver's "raw"), so both loops register the same rows."""
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser, ScanToMapLocaliser
    from sps_amd.sps_filters import SPSCVMFilter
    from sps_amd.trajectory import ape_translation
    n, step = 8, 0.5
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

    ndt = NDTLocaliser(map64, resolution=RES, leaf=LEAF)
    got, steps = run(ndt)
    want, ref_steps = run(RestatementLocaliser(NR.cells(map64, RES), ndt))
    icp, _ = run(ScanToMapLocaliser(map64, leaf=LEAF))
    print("APE NDT:", ape_translation(got, truth), " APE ICP (same frames, for the record):", ape_translation(icp, truth))
    for i in range(n):
        a, b = steps[i].pose_result, ref_steps[i].pose_result
        dt, dr = LR.pose_difference(got[i], want[i])
        print(f"frame {i}: status {a.status}/{b.status} iterations {a.iterations}/{b.iterations} count {a.n_corr}/{b.n_corr} "
              f"device vs restatement {dt:.3e} m {dr:.3e} rad")
        assert (a.status, a.iterations, a.n_corr, a.n_points) == (b.status, b.iterations, b.n_corr, b.n_points), i
        assert dt <= full["tol_t"] and dr <= full["tol_r"], i
    ndt.ctx.check_errors(stream())
