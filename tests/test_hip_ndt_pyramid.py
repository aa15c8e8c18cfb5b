"""GPU tests of the multi-resolution NDT alignment (sps_amd.localiser.NDTLocaliser(..., resolutions=...); C ABI: the "NDT
localiser, multi-resolution pyramid" section of include/sps_hip.h) against single-map localisers chained from the host and
against the numpy restatement in tests/ndt_pyramid_reference.py.  The scene is test_hip_ndt.py's: 400 x 32 rays, the
synthetic map, scan 1 thinned at leaf 0.4 to 4 157 points; the start is 0.5 m off along the corridor, where the 1 m map
alone does not recover (tests/test_ndt_pyramid_cpu.py)."""
import math

import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_pyramid_reference as PR
from tests import ndt_reference as NR
from tests.helpers import CFG, net_from_params, straddle_params
from tests.test_ndt_cpu import KW, LEAF, T_INIT, T_TRUE, sensor_scan

pytestmark = pytest.mark.gpu

RESOLUTIONS = (2.0, 1.0, 0.5)
T_START = LR.perturbation(0.5, 0.0, 0.0, 0.0) @ T_TRUE
# this project's rule for float64 comparisons that differ only in the order of a sum (test_hip_localiser.py)
TOL_FLOOR = 1e-12


@pytest.fixture(scope="module")
def map_xyz():
    return synthetic.build_map(**KW)[:, :3].astype(np.float64)


@pytest.fixture(scope="module")
def cmaps(map_xyz):
    return PR.pyramid(map_xyz, RESOLUTIONS)


@pytest.fixture(scope="module")
def pyr(map_xyz):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(map_xyz, resolutions=RESOLUTIONS, leaf=LEAF, iterations=90, level_iterations=(30, 30, 30))


@pytest.fixture(scope="module")
def singles(map_xyz):
    """one plain localiser per resolution"""
    from sps_amd.localiser import NDTLocaliser
    return [NDTLocaliser(map_xyz, resolution=r, leaf=LEAF) for r in RESOLUTIONS]


def spread_tolerance(fwd, rev):
    """100 x the restatement's own forward-versus-reversed spread on the input, floored"""
    st, sr = LR.pose_difference(fwd["pose"], rev["pose"])
    return st, sr, max(100.0 * st, TOL_FLOOR), max(100.0 * sr, TOL_FLOOR)


@pytest.fixture(scope="module")
def full(cmaps):
    """the restatement's alignment of scan 1 from T_START, forward and reversed, and the pose tolerance that follows"""
    scan = sensor_scan(1)
    _, pts = LR.downsample(scan, len(scan), LEAF)
    kw = dict(iters=90, level_iters=(30, 30, 30))
    fwd = PR.align(pts, cmaps, T_START, **kw)
    rev = PR.align(pts, cmaps, T_START, reverse=True, **kw)
    st, sr, tol_t, tol_r = spread_tolerance(fwd, rev)
    print(f"spread forward/reversed: {st:.3e} m {sr:.3e} rad -> tolerance {tol_t:.3e} m {tol_r:.3e} rad")
    return dict(scan=scan, pts=pts, fwd=fwd, rev=rev, tol_t=tol_t, tol_r=tol_r)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    assert (a.status, a.iterations, a.n_corr, a.n_points) == (b.status, b.iterations, b.n_corr, b.n_points)
    for x, y in ((a.pose, b.pose), (a.trace, b.trace), (a.normal, b.normal), (a.levels, b.levels)):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()


def status_words(loc, scan, T, **kw):
    """the four status words of a call, which PoseResult does not show in full: (code, slots, count, level)"""
    pend = loc.submit(scan, len(scan), T, **kw)
    res = pend.result()
    o = pend._layout()
    return res, [int(v) for v in pend._host.numpy()[o["status"]:o["n_points"]].view(np.int32)]


# ---- the maps --------------------------------------------------------------------------------------------------------------
def test_every_level_is_the_single_map_of_its_resolution(pyr, singles):
    for l, one in enumerate(singles):
        got, want = pyr.pyramid_cells(l), one.map_cells()
        assert len(got[0]) == one.n_cells == pyr.level_cells[l] > 0
        for g, w in zip(got, want):                                        # keys, counts, means, inverse covariances, valid flags
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert pyr.level_cells[0] < pyr.level_cells[1] < pyr.level_cells[2]
    # the single map beside the pyramid is the one `resolution` asks for, untouched
    for g, w in zip(pyr.map_cells(), singles[1].map_cells()):
        assert g.tobytes() == w.tobytes()
    with pytest.raises(ValueError):
        pyr.pyramid_cells(3)
    with pytest.raises(ValueError):
        singles[0].pyramid_cells(0)


# ---- against single-map localisers -----------------------------------------------------------------------------------------
def test_one_level_is_the_single_call(map_xyz, singles, full):
    from sps_amd.localiser import NDTLocaliser
    one = NDTLocaliser(map_xyz, resolutions=(1.0,), leaf=LEAF)
    scan = dev(full["scan"])
    a, words = status_words(one, scan, T_INIT, with_normal=True)
    b = singles[1](scan, len(scan), T_INIT, with_normal=True)
    assert b.status == 0 and 1 < b.iterations < 30
    assert (a.status, a.iterations, a.n_corr, a.n_points) == (b.status, b.iterations, b.n_corr, b.n_points)
    assert words[:3] == [b.status, b.iterations, b.n_corr] and words[3] == 0
    assert a.pose.tobytes() == b.pose.tobytes() and a.trace.tobytes() == b.trace.tobytes()
    assert a.normal.tobytes() == b.normal.tobytes()
    assert b.levels is None and len(a.levels) == a.iterations and not a.levels.any()
    one.ctx.check_errors(stream())


@pytest.mark.parametrize("caps", [(30, 30, 30), (5, 3, 30), (1, 1, 1)])
def test_three_levels_are_three_chained_calls(map_xyz, singles, full, caps):
    """budget = the sum of the caps, so no level is cut short by it: the pose and the rows of every slot are those of three
    plain localisers run one after another with iterations = caps[l], each from the end pose of the one before"""
    from sps_amd.localiser import NDTLocaliser
    loc = NDTLocaliser(map_xyz, resolutions=RESOLUTIONS, leaf=LEAF, iterations=sum(caps), level_iterations=caps)
    scan = dev(full["scan"])
    got, words = status_words(loc, scan, T_START, with_normal=True)
    T, chain = T_START, []
    for one, cap in zip(singles, caps):
        r = one(scan, len(scan), T, with_normal=True, iterations=cap)
        assert r.status in (0, 1)                                          # the input's condition: no level fails
        chain.append(r)
        T = r.pose
    print(f"caps {caps}: chained status/iterations " + ", ".join(f"{r.status}/{r.iterations}" for r in chain)
          + f"; pyramid status {got.status}, {got.iterations} slots")
    assert got.pose.tobytes() == chain[-1].pose.tobytes()
    assert got.trace.tobytes() == np.concatenate([r.trace for r in chain]).tobytes()
    assert got.normal.tobytes() == np.concatenate([r.normal for r in chain]).tobytes()
    assert list(got.levels) == sum(([l] * r.iterations for l, r in enumerate(chain)), [])
    assert words == [chain[-1].status, sum(r.iterations for r in chain), chain[-1].n_corr, 2]
    assert got.n_points == chain[0].n_points == len(full["pts"])
    if caps == (5, 3, 30):
        assert [r.status for r in chain[:2]] == [1, 1]                     # both handoffs were forced by the cap
    loc.ctx.check_errors(stream())


# ---- against the restatement -----------------------------------------------------------------------------------------------
def test_full_alignment_matches_the_restatement(pyr, full):
    fwd, tol_t, tol_r = full["fwd"], full["tol_t"], full["tol_r"]
    res, words = status_words(pyr, dev(full["scan"]), T_START)
    # exact counts need an input without a point on a cell face and without a weight on the guard's boundary
    assert fwd["faces"] == 0 and fwd["boundary"] == 0
    assert fwd["status"] == 0 and set(fwd["levels"]) == {0, 1, 2}
    assert words == [fwd["status"], fwd["iterations"], fwd["n_corr"], fwd["level"]]
    np.testing.assert_array_equal(res.levels, fwd["levels"])
    np.testing.assert_array_equal(res.trace[:, 0], fwd["trace"][:, 0])    # the count of every slot
    dt, dr = LR.pose_difference(res.pose, fwd["pose"])
    print(f"device vs restatement: {dt:.3e} m {dr:.3e} rad")
    assert dt <= tol_t and dr <= tol_r
    et, er = LR.pose_difference(res.pose, T_TRUE)
    print(f"error against the ground truth: {et:.6e} m {er:.6e} rad after {res.iterations} slots, levels "
          f"{np.bincount(res.levels, minlength=3)}")
    assert et < 0.02                                                       # test_ndt_pyramid_cpu.py's bound


def test_two_calls_give_the_same_bits(pyr):
    scan = dev(sensor_scan(2))
    a = pyr(scan, len(scan), T_START, with_normal=True)
    b = pyr(scan, len(scan), T_START, with_normal=True)
    assert a.iterations > 3 and len(set(a.levels)) == 3
    same_bits(a, b)


# ---- edges -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(map_xyz):
    """a small capacity, few slots and a low count limit: for scans of a workgroup's size"""
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(map_xyz, resolutions=RESOLUTIONS, leaf=LEAF, iterations=6, level_iterations=(2, 2, 2),
                        min_correspondences=10, capacity=1000)


@pytest.mark.parametrize("n", [0, 31, 32, 33, 1000])
def test_scan_counts_around_a_workgroup(small, cmaps, full, n):
    """a workgroup of launch A covers 32 points; 1000 is the localiser's capacity.  The rows are thinned points already, so
    the first n of them are the n points that enter the alignment (for 1000: the whole scan, cut at the capacity)."""
    pts = full["pts"][:n]
    rows = full["scan"] if n == 1000 else np.c_[pts, np.zeros(len(pts))].astype(np.float32)
    kw = dict(iters=6, level_iters=(2, 2, 2), min_corr=10)
    fwd = PR.align(pts, cmaps, T_START, **kw)
    rev = PR.align(pts, cmaps, T_START, reverse=True, **kw)
    st, sr, tol_t, tol_r = spread_tolerance(fwd, rev)
    assert fwd["faces"] == 0 and fwd["boundary"] == 0
    res, words = status_words(small, dev(rows) if len(rows) else torch.zeros((0, 4), dtype=torch.float32, device="cuda"), T_START)
    dt, dr = LR.pose_difference(res.pose, fwd["pose"])
    print(f"n {n}: status {res.status} slots {res.iterations} levels {list(res.levels)} counts {list(res.trace[:, 0])}; spread "
          f"{st:.3e} m {sr:.3e} rad; device vs restatement {dt:.3e} m {dr:.3e} rad")
    assert res.n_points == n
    assert words == [fwd["status"], fwd["iterations"], fwd["n_corr"], fwd["level"]]
    np.testing.assert_array_equal(res.levels, fwd["levels"])
    np.testing.assert_array_equal(res.trace[:, 0], fwd["trace"][:, 0])
    assert dt <= tol_t and dr <= tol_r
    if n == 0:
        assert (res.status, res.iterations) == (2, 1) and res.pose.tobytes() == T_START.tobytes()
    small.ctx.check_errors(stream())


def test_an_empty_map_gives_status_2(full):
    from sps_amd.localiser import NDTLocaliser
    empty = NDTLocaliser(np.zeros((0, 3)), resolutions=RESOLUTIONS, leaf=LEAF)
    res, words = status_words(empty, dev(full["scan"]), T_START)
    assert words == [2, 1, 0, 0] and res.n_points == len(full["pts"]) and list(res.levels) == [0]
    assert res.pose.tobytes() == T_START.tobytes()
    assert all(len(empty.pyramid_cells(l)[0]) == 0 for l in range(3))
    empty.ctx.check_errors(stream())


def test_a_coarsest_level_without_cells_gives_status_2(map_xyz, full):
    """through the C ABI: a second build replaces the pyramid by one whose level 0 has no cells and whose finer levels are
    the real ones.  Status 2 at level 0 is final: the finer levels are never entered."""
    from sps_amd.datasets.blt_dataset import radius_grid_cells
    from sps_amd.localiser import NDTLocaliser
    loc = NDTLocaliser(map_xyz, resolutions=RESOLUTIONS, leaf=LEAF, iterations=90)
    scan = dev(full["scan"])
    before = loc(scan, len(scan), T_START)
    assert before.status == 0
    xyz = dev(map_xyz)
    groups = [radius_grid_cells(xyz, r) for r in RESOLUTIONS]
    groups = [(k.contiguous(), s, p) for k, s, p in groups]
    levels = [(k.data_ptr(), s.data_ptr(), p.data_ptr(), 0 if l == 0 else len(k), r)
              for l, ((k, s, p), r) in enumerate(zip(groups, RESOLUTIONS))]
    loc.ctx.ndt_pyramid_build(levels, xyz.data_ptr(), len(xyz), loc.min_points_per_cell, loc.eig_ratio, loc.outlier_ratio, stream())
    loc.level_cells = tuple(lv[3] for lv in levels)
    res, words = status_words(loc, scan, T_START)
    assert words == [2, 1, 0, 0] and list(res.levels) == [0] and res.pose.tobytes() == T_START.tobytes()
    assert len(loc.pyramid_cells(0)[0]) == 0 and len(loc.pyramid_cells(2)[0]) == len(groups[2][0])
    loc.ctx.check_errors(stream())


def test_a_level_that_converges_in_the_last_slot_hands_over_to_nobody(pyr, full):
    per = full["fwd"]["per_level"]
    k = per[0]["iterations"]
    assert per[0]["status"] == 0 and 1 < k < 30                            # level 0 converges in slot k - 1
    res, words = status_words(pyr, dev(full["scan"]), T_START, iterations=k)
    assert words[:2] == [1, k] and words[3] == 0 and not res.levels.any()  # exhausted; the finer levels were not entered
    assert res.trace[-1, 2] < pyr.tol_t and res.trace[-1, 3] < pyr.tol_r   # although its last step was a converged one
    nxt = pyr(dev(full["scan"]), len(full["scan"]), T_START, iterations=k + 1)
    assert list(nxt.levels) == [0] * k + [1] and nxt.status == 1
    assert nxt.trace[:k].tobytes() == res.trace.tobytes()


def test_bad_rows_are_skipped(pyr):
    scan = sensor_scan(3)
    bad = [17, 400, 4000]
    rows = scan.copy()
    rows[17, 0], rows[400, 2], rows[4000, 1] = np.nan, 3.0e6, -np.inf
    clean = np.delete(scan, bad, axis=0)
    a = pyr(dev(rows), len(rows), T_START, with_normal=True)
    b = pyr(dev(clean), len(clean), T_START, with_normal=True)            # the survivors and their order are the same
    assert a.status in (0, 1) and a.n_corr > 1000 and len(set(a.levels)) == 3
    same_bits(a, b)
    pyr.ctx.check_errors(stream())                                         # never a sticky error


def test_arguments_are_checked(pyr, full):
    from sps_amd import _native
    scan = dev(full["scan"])
    with pytest.raises(ValueError):
        pyr.submit(scan, len(scan), T_START, integrate=True)
    c = pyr.ctx
    out = torch.zeros(64, dtype=torch.float64, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    args = (out.data_ptr(), out.data_ptr() + 128, out.data_ptr() + 160, None, out.data_ptr() + 320, pyr._pyr_scratch.data_ptr(), stream())
    for caps, neighbours in (((30, 30, 0), 7), ((30, 30, 30), 5)):
        with pytest.raises(_native.SpsError):
            c.ndt_pyramid_align(pyr._pts.data_ptr(), n.data_ptr(), pyr.capacity, T_START, 2, caps, neighbours, 50, 1e-4, 1e-5, *args)
    plain = _native.Context(0)
    with pytest.raises(_native.SpsError, match="sps_ndt_pyramid_build has not been called"):
        plain.ndt_pyramid_align(pyr._pts.data_ptr(), n.data_ptr(), pyr.capacity, T_START, 2, (30,), 7, 50, 1e-4, 1e-5, *args)
    with pytest.raises(_native.SpsError):                                  # not strictly decreasing
        plain.ndt_pyramid_build([(None, None, None, 0, 1.0), (None, None, None, 0, 1.0)], None, 0, 6, 0.01, 0.55, stream())


# ---- stream order: the filter's pending frame goes straight in -------------------------------------------------------------
def test_submit_filtered_equals_result_then_submit(pyr, map_xyz):
    from sps_amd.sps_filters import SPSFilter
    params = straddle_params(O.random_params(seed=0), synthetic.small_scene(seed=11, n_scan=2500))
    net = net_from_params(params).cuda().eval().freeze()
    f = SPSFilter(net, map_xyz.astype(np.float32), voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=CFG["FILTER"]["THRESHOLD"])
    scan = sensor_scan(4)
    pend = f.submit(scan, T_TRUE)
    pose_pend = pyr.submit_filtered(pend, T_START, with_normal=True)       # queued behind the filter, before the frame's result()
    a = pose_pend.result()                                                 # read only after the event
    fres = pend.result()
    assert 0 < len(fres.filtered) <= len(scan)
    b = pyr(fres.filtered.clone(), len(fres.filtered), T_START, with_normal=True)
    assert a.iterations > 3
    same_bits(a, b)


# ---- the closed loop -------------------------------------------------------------------------------------------------------
class RestatementLocaliser:
    """tests/ndt_pyramid_reference.py behind the interface LocalisationLoop uses"""

    def __init__(self, cmaps, like):
        self.cmaps, self.like, self.device = cmaps, like, like.device

    def submit_filtered(self, pending, T_init):
        from sps_amd.localiser import PoseResult
        n = int(pending.count_dev.item())
        rows = pending._filtered[:n].cpu().numpy()
        L = self.like
        _, pts = LR.downsample(rows, n, L.leaf, L.capacity)
        r = PR.align(pts, self.cmaps, T_init, L.iterations, L.level_iterations, L.neighbours, L.min_correspondences,
                     L.outlier_ratio, L.tol_t, L.tol_r)
        res = PoseResult(r["pose"], r["status"], r["iterations"], r["n_corr"], float("nan"), r["trace"], None, len(pts), None,
                         r["levels"])

        class Done:
            def result(self):
                return res
        return Done()


def test_closed_loop_follows_the_restatement():
    """LocalisationLoop(SPSCVMFilter, pyramid localiser) over the 8 synthetic frames of the driver's --synthetic 8 replay, at
    epsilon = 2 (every point passes), against the same loop driven by the restatement: status, slots, levels and counts of
    every frame.  The pose difference is printed only: a frame starts from the poses before it, so it is not bounded by
    the spread of one alignment."""
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser
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

    ndt = NDTLocaliser(map64, resolutions=RESOLUTIONS, leaf=LEAF)
    got, steps = run(ndt)
    want, ref_steps = run(RestatementLocaliser(PR.pyramid(map64, RESOLUTIONS), ndt))
    print("APE pyramid:", ape_translation(got, truth))
    for i in range(n):
        a, b = steps[i].pose_result, ref_steps[i].pose_result
        dt, dr = LR.pose_difference(got[i], want[i])
        print(f"frame {i}: status {a.status}/{b.status} slots {a.iterations}/{b.iterations} levels "
              f"{np.bincount(a.levels, minlength=3)}/{np.bincount(b.levels, minlength=3)} count {a.n_corr}/{b.n_corr} "
              f"device vs restatement {dt:.3e} m {dr:.3e} rad")
        assert (a.status, a.iterations, a.n_corr, a.n_points) == (b.status, b.iterations, b.n_corr, b.n_points), i
        np.testing.assert_array_equal(a.levels, b.levels)
    ndt.ctx.check_errors(stream())
