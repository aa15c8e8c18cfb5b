"""GPU tests of the NDT pose search (sps_amd.localiser.NDTLocaliser.score_poses / relocalise; C ABI: the "NDT localiser,
pose search" section of include/sps_hip.h) against sps_ndt_align_batch with no iterations, bit for bit, and against the
numpy restatement in tests/ndt_search_reference.py.  The scene is test_hip_ndt.py's (400 x 32 rays, ~4.2 k points after
thinning), the grid the 75 poses of tests/test_ndt_search_cpu.py."""
import math

import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_batch_reference as NB
from tests import ndt_reference as NR
from tests import ndt_search_reference as NS
from tests.helpers import CFG, net_from_params
from tests.test_ndt_cpu import KW, LEAF
from tests.test_ndt_search_cpu import ACROSS, ALONG, KEEP, YAW, search75

pytestmark = pytest.mark.gpu

RES = 1.0
TOL_FLOOR = 1e-12      # this project's rule for float64 comparisons that differ only in the order of a sum
TILE = 32              # NDT_SCORE_TILE


@pytest.fixture(scope="module")
def scene():
    return search75()


@pytest.fixture(scope="module")
def loc(scene):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF)


@pytest.fixture(scope="module")
def loc1(scene):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF, neighbours=1)


@pytest.fixture(scope="module")
def scores75(loc, scene):
    """the grid's scores on the device, computed once"""
    scan = dev(scene["scan"])
    return loc.score_poses(scan, len(scan), scene["poses"]).result()


@pytest.fixture(scope="module")
def reloc75(loc, scene):
    scan = dev(scene["scan"])
    return loc.relocalise(scan, len(scan), scene["poses"], keep=KEEP, with_normal=True).result()


@pytest.fixture(scope="module")
def tol(scene):
    """the pose tolerance of test_hip_ndt.py: 100 x the restatement's forward / reversed spread, floored at 1e-12"""
    start = scene["ref"]["starts"][0]
    fwd = scene["ref"]["batch"]["results"][0]
    rev = NR.align(scene["pts"], scene["cmap"], start, reverse=True)
    spread_t, spread_r = LR.pose_difference(fwd["pose"], rev["pose"])
    t = max(100.0 * spread_t, TOL_FLOOR), max(100.0 * spread_r, TOL_FLOOR)
    print(f"spread forward/reversed: {spread_t:.3e} m {spread_r:.3e} rad -> tolerance {t[0]:.3e} m {t[1]:.3e} rad")
    return t


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    assert (a.status, a.iterations, a.n_corr, a.n_points) == (b.status, b.iterations, b.n_corr, b.n_points)
    for x, y in ((a.pose, b.pose), (a.trace, b.trace), (a.normal, b.normal)):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()


def same_batch(a, b):
    assert len(a.results) == len(b.results) and a.best == b.best
    for x, y in zip(a.results, b.results):
        same_bits(x, y)
    assert a.scores.tobytes() == b.scores.tobytes() and a.counts.tobytes() == b.counts.tobytes()
    assert a.pose.tobytes() == b.pose.tobytes()


def raw_scores(L, pts, n, cap, poses, neighbours=None):
    """sps_ndt_score_poses itself on points given as they are: [P, 2] (score, count)"""
    from sps_amd import _native
    P = len(poses)
    p = dev(np.asarray(pts, dtype=np.float64).reshape(-1, 3)) if len(pts) else torch.zeros((1, 3), dtype=torch.float64, device="cuda")
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    T = dev(np.asarray(poses, dtype=np.float64))
    out = torch.full((P, 2), -7.0, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(_native.lib.sps_ndt_score_scratch(cap, P), dtype=torch.uint8, device="cuda")
    L.ctx.ndt_score_poses(p.data_ptr(), n_dev.data_ptr(), cap, T.data_ptr(), P, L.neighbours if neighbours is None else neighbours,
                          L.outlier_ratio, out.data_ptr(), scratch.data_ptr(), stream())
    return out.cpu().numpy()


def raw_batch0(L, pts, n, cap, poses):
    """final_dev [K, 2] of sps_ndt_align_batch(iters = 0) on the same points"""
    from sps_amd import _native
    K = len(poses)
    p = dev(np.asarray(pts, dtype=np.float64).reshape(-1, 3)) if len(pts) else torch.zeros((1, 3), dtype=torch.float64, device="cuda")
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    T = dev(np.asarray(poses, dtype=np.float64))
    T_out = torch.zeros((K, 16), dtype=torch.float64, device="cuda")
    status = torch.zeros((K, 4), dtype=torch.int32, device="cuda")
    final = torch.full((K, 2), -7.0, dtype=torch.float64, device="cuda")
    best = torch.zeros(4, dtype=torch.int32, device="cuda")
    T_best = torch.zeros(16, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(_native.lib.sps_ndt_align_batch_scratch(cap, K), dtype=torch.uint8, device="cuda")
    L.ctx.ndt_align_batch(p.data_ptr(), n_dev.data_ptr(), cap, T.data_ptr(), K, 0, L.neighbours, L.min_correspondences,
                          L.outlier_ratio, L.tol_t, L.tol_r, T_out.data_ptr(), status.data_ptr(), None, None, final.data_ptr(),
                          best.data_ptr(), T_best.data_ptr(), scratch.data_ptr(), stream())
    return final.cpu().numpy()


def raw_top(L, table, poses, min_corr, k):
    """sps_ndt_top_poses itself: (indices [k], T_top [k, 4, 4], n_top)"""
    sc = dev(np.asarray(table, dtype=np.float64))
    T = dev(np.asarray(poses, dtype=np.float64))
    idx = torch.full((k,), -9, dtype=torch.int32, device="cuda")
    T_top = torch.zeros((k, 4, 4), dtype=torch.float64, device="cuda")
    n_top = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    L.ctx.ndt_top_poses(sc.data_ptr(), T.data_ptr(), len(table), min_corr, k, idx.data_ptr(), T_top.data_ptr(), n_top.data_ptr(),
                        stream())
    return idx.cpu().numpy().astype(np.int64), T_top.cpu().numpy(), int(n_top.item())


# ---- a score is the final score of a batch without iterations ---------------------------------------------------------------
@pytest.mark.parametrize("neighbours", [7, 1])
def test_score_poses_equals_the_zero_iteration_batch(loc, loc1, scene, neighbours):
    L = loc if neighbours == 7 else loc1
    scan = dev(scene["scan"])
    scores, counts = L.score_poses(scan, len(scan), scene["poses"]).result()
    assert scores.shape == (75,) and scores.dtype == np.float64 and counts.shape == (75,) and counts.dtype == np.int64
    for lo in (0, 11):                                                      # 64 poses at a time, all 75 between them
        b = L.submit_batch(scan, len(scan), scene["poses"][lo:lo + 64], iterations=0).result()
        assert all(r.iterations == 0 for r in b.results)
        assert b.scores.tobytes() == scores[lo:lo + 64].tobytes()
        assert b.counts.tobytes() == counts[lo:lo + 64].tobytes()
    assert len(set(scores.tolist())) == 75 and counts.max() > 1000
    L.ctx.check_errors(stream())


@pytest.mark.parametrize("neighbours", [7, 1])
def test_scores_match_the_restatement(loc, loc1, scene, neighbours):
    """The device adds the m terms of a pose in its fixed order, the restatement with math.fsum: the bound is
    (m + blocks + 40) * 2^-52 * sum |term| (ndt_search_reference.sum_bound).  Counts are exact: no point of the input
    lies on a cell face."""
    L = loc if neighbours == 7 else loc1
    scan = dev(scene["scan"])
    scores, counts = L.score_poses(scan, len(scan), scene["poses"]).result()
    g = scene["grid"] if neighbours == 7 else NS.score_poses(scene["pts"], scene["cmap"], scene["poses"], neighbours=1)
    n = len(scene["pts"])
    assert g["faces"].sum() == 0
    worst = 0.0
    for k in range(75):
        bound = NS.sum_bound(g["m"][k], n, g["sum_abs"][k])
        worst = max(worst, abs(scores[k] - g["scores"][k]) / bound)
        assert counts[k] == g["counts"][k], k
        assert abs(scores[k] - g["scores"][k]) <= bound, (k, scores[k], g["scores"][k], bound)
    print(f"neighbours {neighbours}: largest |device - fsum| / bound = {worst:.3f}")


# ---- shapes at the edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap", [(0, 8), (1, 1), (1, 40), (32, 32), (32, 64), (33, 32), (33, 33), (33, 70), (100, 33)])
@pytest.mark.parametrize("P", [1, TILE + 1])
def test_edge_shapes(loc, scene, n, cap, P):
    """n points in the device count, room for cap: min(n, cap) are scored.  Against the batch without iterations bit for
    bit, and against the restatement's counts."""
    have = max(n, cap)
    pts = scene["pts"][7:7 + have]
    poses = scene["poses"][20:20 + P]
    got = raw_scores(loc, pts, n, cap, poses)
    want = raw_batch0(loc, pts, n, cap, poses)
    assert got.tobytes() == want.tobytes()
    used = pts[:min(n, cap)]
    ref = NS.score_poses(used, scene["cmap"], poses)
    np.testing.assert_array_equal(got[:, 1], ref["counts"])
    for k in range(P):
        assert abs(got[k, 0] - ref["scores"][k]) <= NS.sum_bound(ref["m"][k], len(used), ref["sum_abs"][k]), k
    if n == 0:
        assert (got == 0.0).all()
    loc.ctx.check_errors(stream())


def test_off_map_nan_and_identical_poses(loc, scene, scores75):
    poses = scene["poses"][[26, 3, 26, 5, 7]].copy()
    poses[1, 0, 3] += 5000.0                                                # every point off the map
    poses[3, 1, 1] = np.nan                                                 # a NaN entry
    pts = scene["pts"]
    got = raw_scores(loc, pts, len(pts), len(pts), poses)
    assert got[1].tolist() == [0.0, 0.0] and got[3].tolist() == [0.0, 0.0]
    assert got[0].tobytes() == got[2].tobytes() and got[0, 0] == scores75[0][26] and got[0, 1] == scores75[1][26]
    assert got[4, 0] == scores75[0][7]
    idx, T_top, n_top = raw_top(loc, got, poses, loc.min_correspondences, 5)
    assert idx.tolist() == [0, 2, 4, -1, -1] and n_top == 3                 # equal bits: the lower index first; NaN, off-map: never
    assert T_top[0].tobytes() == T_top[1].tobytes() == poses[0].tobytes() and T_top[2].tobytes() == poses[4].tobytes()
    assert T_top[3].tobytes() == T_top[4].tobytes() == poses[0].tobytes()   # the fill rule
    with pytest.raises(ValueError):
        loc.score_poses(dev(scene["scan"]), len(scene["scan"]), poses)      # the Python layer refuses non-finite poses
    loc.ctx.check_errors(stream())


def test_an_empty_map_and_an_empty_scan(scene):
    from sps_amd.localiser import NDTLocaliser
    scan = dev(scene["scan"])
    empty = NDTLocaliser(np.zeros((0, 3)), resolution=RES, leaf=LEAF)
    scores, counts = empty.score_poses(scan, len(scan), scene["poses"][:40]).result()
    assert (scores == 0.0).all() and (counts == 0).all()
    r = empty.relocalise(scan, len(scan), scene["poses"][:40], keep=3).result()
    assert r.index == -1 and not r.ok and r.candidates.tolist() == [-1, -1, -1] and r.batch.best == -1
    assert r.pose.tobytes() == scene["poses"][0].tobytes()
    assert [x.status for x in r.batch.results] == [2, 2, 2]
    empty.ctx.check_errors(stream())


def test_a_grid_longer_than_one_chunk_of_poses(loc, scene, scores75):
    """At the default capacity 2^16 the host walks the poses in chunks of 2 048 (64 MiB of partial rows): 2 048 + 33 poses make
    a second chunk of one whole tile and one pose.  Poses from both chunks and across the seam equal the batch without
    iterations bit for bit, and the first 75 are the grid's."""
    from sps_amd import _native
    P = 2048 + 33
    assert loc.capacity == 1 << 16
    assert _native.lib.sps_ndt_score_scratch(loc.capacity, P) == 2048 * 2048 * 16      # one chunk's rows, not P's
    poses = scene["poses"][np.arange(P) % 75].copy()
    poses[:, 0, 3] += 1e-3 * (np.arange(P) // 75)                           # every pose its own; the first 75 unchanged
    scan = dev(scene["scan"])
    scores, counts = loc.score_poses(scan, len(scan), poses).result()
    assert scores[:75].tobytes() == scores75[0].tobytes() and counts[:75].tobytes() == scores75[1].tobytes()
    for lo in (0, 1984, 2016, P - 64):                                      # first 64, up to the seam, across it, last 64
        b = loc.submit_batch(scan, len(scan), poses[lo:lo + 64], iterations=0).result()
        assert b.scores.tobytes() == scores[lo:lo + 64].tobytes(), lo
        assert b.counts.tobytes() == counts[lo:lo + 64].tobytes(), lo
    assert len(set(scores[2040:].tolist())) == P - 2040 and counts[2040:].min() > 1000   # no row of the seam left unwritten
    r = loc.relocalise(scan, len(scan), poses, keep=4).result()             # and the search downstream of two chunks
    want, n_top = NS.top(scores, counts, loc.min_correspondences, 4)
    assert r.scores.tobytes() == scores.tobytes() and r.candidates.tolist() == want.tolist() and n_top == 4
    loc.ctx.check_errors(stream())


# ---- the top-K rule ---------------------------------------------------------------------------------------------------------
def test_top_poses_equals_the_restatement(loc, scene, scores75):
    scores, counts = scores75
    poses = scene["poses"]
    nan = float("nan")
    rng = np.random.default_rng(11)
    big = np.c_[rng.integers(0, 40, 3000).astype(np.float64), rng.integers(40, 60, 3000).astype(np.float64)]   # many ties
    big[::17, 0] = nan
    tables = [(np.c_[scores, counts.astype(np.float64)], 50, 8), (np.c_[scores, counts.astype(np.float64)], 50, 64),
              (np.c_[scores, counts.astype(np.float64)], 3780, 8),          # few qualify: the fill rule
              (np.c_[scores, counts.astype(np.float64)], 100000, 4),        # nobody qualifies
              (np.array([[3.0, 100], [1.0, 100], [3.0, 100], [3.0, 100]]), 50, 3),
              (np.array([[3.0, 100], [nan, 100], [2.0, 100], [nan, 100]]), 50, 4),
              (np.array([[9.0, 49], [3.0, 50], [2.0, 51]]), 50, 3), (np.array([[1.0, 100], [2.0, 100]]), 50, 5),
              (np.array([[1.0, 10], [2.0, 10]]), 50, 3), (np.array([[0.0, 0]]), 0, 1), (big, 50, 64), (big, 50, 1)]
    for t, (table, min_corr, k) in enumerate(tables):
        P = len(table)
        T = poses[np.arange(P) % 75].copy()
        T[:, 2, 3] = np.arange(P)                                           # every pose its own
        want, n_want = NS.top(table[:, 0], table[:, 1], min_corr, k)
        idx, T_top, n_top = raw_top(loc, table, T, min_corr, k)
        assert idx.tolist() == want.tolist() and n_top == n_want, t
        assert T_top.tobytes() == NS.top_poses(T, want).tobytes(), t
    assert NS.top(scores, counts, 3780, 8)[1] in range(1, 8)                # the third table does exercise the fill rule
    loc.ctx.check_errors(stream())


# ---- relocalise -------------------------------------------------------------------------------------------------------------
def test_relocalise_is_score_top_and_batch(loc, scene, scores75, reloc75):
    scan = dev(scene["scan"])
    scores, counts = scores75
    r = reloc75
    assert r.scores.tobytes() == scores.tobytes() and r.counts.tobytes() == counts.tobytes()
    want, n_top = NS.top(scores, counts, loc.min_correspondences, KEEP)     # the stated rule, on the host
    assert r.candidates.tolist() == want.tolist() and n_top == KEEP
    b = loc.submit_batch(scan, len(scan), scene["poses"][want], with_normal=True).result()
    same_batch(r.batch, b)
    assert r.index == want[b.best] and r.pose.tobytes() == b.pose.tobytes() == b.results[b.best].pose.tobytes() and r.ok
    loc.ctx.check_errors(stream())


def test_relocalise_matches_the_restatement(scene, reloc75, tol):
    r, ref = reloc75, scene["ref"]
    assert r.candidates.tolist() == ref["candidates"].tolist()
    n = len(scene["pts"])
    for k, (a, b) in enumerate(zip(r.batch.results, ref["batch"]["results"])):
        dt, dr = LR.pose_difference(a.pose, b["pose"])
        print(f"candidate {k} (pose {r.candidates[k]}): status {a.status}/{b['status']} iterations {a.iterations}/{b['iterations']} "
              f"pose {dt:.3e} m {dr:.3e} rad final score {r.batch.scores[k]!r} / {ref['batch']['scores'][k]!r}")
    for k, (a, b) in enumerate(zip(r.batch.results, ref["batch"]["results"])):
        assert (a.status, a.iterations, a.n_corr) == (b["status"], b["iterations"], b["n_corr"]), k
        dt, dr = LR.pose_difference(a.pose, b["pose"])
        assert dt <= tol[0] and dr <= tol[1], k
        assert r.batch.counts[k] == ref["batch"]["counts"][k], k
    assert r.batch.best == ref["batch"]["best"] and r.index == ref["index"]
    dt, dr = LR.pose_difference(r.pose, ref["pose"])
    assert dt <= tol[0] and dr <= tol[1]
    assert n == r.batch.results[0].n_points


def test_two_calls_give_the_same_bits(loc, scene, scores75, reloc75):
    scan = dev(scene["scan"])
    again = loc.score_poses(scan, len(scan), scene["poses"]).result()
    assert again[0].tobytes() == scores75[0].tobytes() and again[1].tobytes() == scores75[1].tobytes()
    r = loc.relocalise(scan, len(scan), scene["poses"], keep=KEEP, with_normal=True).result()
    assert r.scores.tobytes() == reloc75.scores.tobytes() and r.candidates.tolist() == reloc75.candidates.tolist()
    same_batch(r.batch, reloc75.batch)
    assert r.index == reloc75.index and r.pose.tobytes() == reloc75.pose.tobytes()


def test_a_call_behind_a_kernel_on_the_callers_stream_sees_its_data(loc, scene, scores75, reloc75):
    scan = dev(scene["scan"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rows = torch.zeros_like(scan)
        a = torch.randn((2048, 2048), device="cuda")
        for _ in range(8):
            a = (a @ a).clamp_(-1.0, 1.0)                                   # work in front of the copy
        rows.copy_(scan + a[0, 0] * 0.0)                                    # the rows exist only once the stream gets here
        count = torch.full((1,), len(scan), dtype=torch.int32, device="cuda")
        ps = loc.score_poses(rows, count, scene["poses"])
        pr = loc.relocalise(rows, count, scene["poses"], keep=KEEP, with_normal=True)
    scores, counts = ps.result()
    r = pr.result()
    torch.cuda.current_stream().wait_stream(side)
    assert scores.tobytes() == scores75[0].tobytes() and counts.tobytes() == scores75[1].tobytes()
    same_batch(r.batch, reloc75.batch)
    assert r.candidates.tolist() == reloc75.candidates.tolist() and r.pose.tobytes() == reloc75.pose.tobytes()


def test_relocalise_filtered_equals_result_then_relocalise(loc, scene):
    from sps_amd.sps_filters import SPSFilter
    from tests.helpers import straddle_params
    from tests.test_ndt_cpu import T_TRUE, sensor_scan
    params = straddle_params(O.random_params(seed=0), synthetic.small_scene(seed=11, n_scan=2500))
    net = net_from_params(params).cuda().eval().freeze()
    f = SPSFilter(net, scene["map_xyz"].astype(np.float32), voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=CFG["FILTER"]["THRESHOLD"])
    scan = sensor_scan(4)
    pend = f.submit(scan, T_TRUE)
    a = loc.relocalise_filtered(pend, scene["poses"], keep=4).result()      # before the frame's result()
    fres = pend.result()
    assert 0 < len(fres.filtered) <= len(scan)
    b = loc.relocalise(fres.filtered.clone(), len(fres.filtered), scene["poses"], keep=4).result()
    assert a.scores.tobytes() == b.scores.tobytes() and a.candidates.tolist() == b.candidates.tolist() and a.index == b.index
    same_batch(a.batch, b.batch)


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked(loc, scene):
    from sps_amd import _native
    scan = dev(scene["scan"])
    for bad in (np.zeros((0, 4, 4)), np.eye(4), np.full((2, 4, 4), np.nan), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError):
            loc.score_poses(scan, len(scan), bad)
        with pytest.raises(ValueError):
            loc.relocalise(scan, len(scan), bad)
    many = np.broadcast_to(np.eye(4), (65537, 4, 4))
    with pytest.raises(ValueError):
        loc.score_poses(scan, len(scan), many)
    for keep in (0, 65):
        with pytest.raises(ValueError):
            loc.relocalise(scan, len(scan), scene["poses"], keep=keep)
    with pytest.raises(TypeError):
        loc.score_poses(torch.zeros((4, 4)), 4, scene["poses"])             # a host tensor
    # the C entry points themselves
    pts = torch.zeros((64, 3), dtype=torch.float64, device="cuda")
    n = torch.tensor([64], dtype=torch.int32, device="cuda")
    T = dev(np.tile(np.eye(4), (4, 1, 1)))
    out = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    scratch = torch.zeros(_native.lib.sps_ndt_score_scratch(64, 4), dtype=torch.uint8, device="cuda")
    idx = torch.zeros(64, dtype=torch.int32, device="cuda")
    T_top = torch.zeros((64, 16), dtype=torch.float64, device="cuda")

    def score(ctx, P=4, neighbours=7, outlier=0.55, T_ptr=T.data_ptr()):
        ctx.ndt_score_poses(pts.data_ptr(), n.data_ptr(), 64, T_ptr, P, neighbours, outlier, out.data_ptr(), scratch.data_ptr(), stream())

    def top(P=4, k=2):
        loc.ctx.ndt_top_poses(out.data_ptr(), T.data_ptr(), P, 50, k, idx.data_ptr(), T_top.data_ptr(), n.data_ptr(), stream())

    fresh = _native.Context(torch.cuda.current_device())
    with pytest.raises(_native.SpsError, match="sps_ndt_map_build has not been called") as e:
        score(fresh)
    assert e.value.code == _native.ERR_INVALID
    with pytest.raises(_native.SpsError, match="neighbours must be 1 or 7"):
        score(loc.ctx, neighbours=3)
    for kw in (dict(P=0), dict(P=65537), dict(T_ptr=None), dict(outlier=float("nan")), dict(outlier=1.0)):
        with pytest.raises(_native.SpsError) as e:
            score(loc.ctx, **kw)
        assert e.value.code == _native.ERR_INVALID
    for kw in (dict(P=0), dict(P=65537), dict(k=0), dict(k=65)):
        with pytest.raises(_native.SpsError) as e:
            top(**kw)
        assert e.value.code == _native.ERR_INVALID
    score(loc.ctx)                                                          # and the same arguments in range are accepted
    n2 = torch.zeros(1, dtype=torch.int32, device="cuda")
    loc.ctx.ndt_top_poses(out.data_ptr(), T.data_ptr(), 4, 50, 64, idx.data_ptr(), T_top.data_ptr(), n2.data_ptr(), stream())
    torch.cuda.synchronize()
    assert int(n2.item()) == 0 and (idx.cpu().numpy() == -1).all()
    loc.ctx.check_errors(stream())


# ---- the closed loop --------------------------------------------------------------------------------------------------------
def test_closed_loop_with_search_follows_the_restatement(tol):
    """LocalisationLoop(SPSCVMFilter, NDTLocaliser, search) over the 8 synthetic frames of test_hip_ndt_batch.py's loop test,
    started 1.2 m and 6 degrees off the first true pose: further than a basin (a single registration from there ends about
    a metre off, tests/test_ndt_search_cpu.py shows the same on its scene).  The filter runs at epsilon = 2 (every point
    passes)."""
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser, pose_grid
    from sps_amd.sps_filters import SPSCVMFilter
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
    g = pose_grid(ALONG, ACROSS, YAW)
    centre = (2 * len(ACROSS) + 1) * len(YAW) + 2
    search = np.concatenate([g[[centre]], np.delete(g, centre, axis=0)])
    assert np.array_equal(search[0], np.eye(4)) and len(search) == 75
    start = truth[0] @ NB.offset(1.1, -0.4, 6.0)

    def run(localiser, initial, **kw):
        loop = LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0), localiser, initial, **kw)
        steps = [loop.step(s) for s in scans]
        return loop.poses, steps

    ndt = NDTLocaliser(map64, resolution=RES, leaf=LEAF)
    got, steps = run(ndt, start, search=search)
    want, ref_steps = run(NS.SearchLocaliser(NR.cells(map64, RES), ndt), start, search=search)
    for i in range(n):
        a, b = steps[i], ref_steps[i]
        dt, dr = LR.pose_difference(got[i], want[i])
        et, _ = LR.pose_difference(got[i], truth[i])
        print(f"frame {i}: search {a.search is not None}/{b.search is not None} index "
              f"{a.search.index if a.search else None}/{b.search.index if b.search else None} status "
              f"{a.pose_result.status}/{b.pose_result.status} flagged {a.flagged}/{b.flagged} device vs restatement {dt:.3e} m "
              f"{dr:.3e} rad, error {et:.4f} m")
    assert steps[0].search is not None and ref_steps[0].search is not None
    for i in range(n):
        a, b = steps[i], ref_steps[i]
        assert (a.search is None) == (b.search is None) == (i > 0 and not steps[i - 1].flagged), i
        assert a.flagged == b.flagged and a.pose_result.status == b.pose_result.status, i
        if a.search is not None:
            assert a.search.index == b.search.index and a.search.candidates.tolist() == b.search.candidates.tolist(), i
            assert [r.status for r in a.batch.results] == [r.status for r in b.batch.results], i
            assert a.batch is a.search.batch and a.pose_result is a.batch.results[max(a.batch.best, 0)]
        dt, dr = LR.pose_difference(got[i], want[i])
        assert dt <= tol[0] and dr <= tol[1], i
    assert not steps[0].flagged and LR.pose_difference(got[0], truth[0])[0] < 0.02     # frame 0 ends in the true basin
    # search = None is the loop as it was: the LoopSteps of a loop built without the argument, bit for bit
    plain, plain_steps = run(ndt, truth[0])
    again, again_steps = run(ndt, truth[0], search=None)
    assert all(s.search is None and s.batch is None for s in plain_steps + again_steps)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(plain, again))
    for s, t in zip(plain_steps, again_steps):
        same_bits(s.pose_result, t.pose_result)
        assert s.flagged == t.flagged and s.guess.tobytes() == t.guess.tobytes() and s.pose.tobytes() == t.pose.tobytes()
    ndt.ctx.check_errors(stream())


def test_a_flagged_frame_is_followed_by_a_search(loc, scene):
    """The search runs at the first frame and at every frame directly after a flagged one, whether the flagged frame was
    itself a search or a plain registration.  A scan 5 km off the map is flagged (no point counted); the filter is a stand-in
    that keeps every row."""
    from types import SimpleNamespace
    from sps_amd.localiser import LocalisationLoop, pose_grid
    from tests.test_ndt_cpu import T_TRUE
    from tests.test_ndt_search_cpu import T_CENTRE

    class KeepAll:
        takes_pose = False

        def submit(self, scan):
            return SimpleNamespace(result=lambda: SimpleNamespace(filtered=scan))

    g = pose_grid(ALONG, ACROSS, YAW)
    centre = (2 * len(ACROSS) + 1) * len(YAW) + 2
    search = np.concatenate([g[[centre]], np.delete(g, centre, axis=0)])
    good = scene["scan"]
    far = good.copy()
    far[:, 0] += 5000.0
    loop = LocalisationLoop(KeepAll(), loc, T_CENTRE, search=search, search_keep=KEEP)
    steps = [loop.step(s) for s in (far, good, good, far, good, good)]
    for i, st in enumerate(steps):
        print(f"frame {i}: search {st.search is not None} index {st.search.index if st.search else None} status "
              f"{st.pose_result.status} flagged {st.flagged} error {LR.pose_difference(st.pose, T_TRUE)[0]:.4f} m")
    assert [st.search is not None for st in steps] == [True, True, False, False, True, False]
    assert [st.flagged for st in steps] == [True, False, False, True, False, False]
    # a flagged search: nobody qualifies, the guess is kept
    assert steps[0].search.index == -1 and (steps[0].search.counts == 0).all() and steps[0].pose.tobytes() == T_CENTRE.tobytes()
    assert steps[0].pose_result.status == 2 and steps[0].batch is steps[0].search.batch
    # the search after it is the grid of test_relocalise_*: the same poses in another order, pose 26 of that grid wins
    assert steps[1].guess.tobytes() == T_CENTRE.tobytes() and steps[1].search.index >= 0
    assert (T_CENTRE @ search[steps[1].search.index]).tobytes() == scene["poses"][26].tobytes()
    assert LR.pose_difference(steps[1].pose, T_TRUE)[0] < 0.02
    # a flagged plain registration keeps its guess, and the next frame searches around the loop's guess
    assert steps[3].search is None and steps[3].batch is None and steps[3].pose_result.status == 2
    assert steps[3].pose.tobytes() == steps[3].guess.tobytes()
    direct = loc.relocalise(dev(good), len(good), np.stack([steps[4].guess @ d for d in search]), keep=KEEP).result()
    assert steps[4].search.index == direct.index >= 0 and steps[4].pose.tobytes() == direct.pose.tobytes()
    loc.ctx.check_errors(stream())
