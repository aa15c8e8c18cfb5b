"""GPU tests of the coarse-to-fine NDT alignment from several start poses (C ABI: the "NDT localiser, pyramid, several
hypotheses" section of include/sps_hip.h; sps_amd.localiser.NDTLocaliser.submit_batch / submit_from_device / relocalise with
coarse_to_fine=True).  Almost every comparison is for equal bytes against an entry point that existed before:
sps_ndt_pyramid_align per hypothesis, sps_ndt_align_batch for a pyramid of one level, sps_ndt_score_poses for the final
scores, submit(..., integrate=True, carve=True) of a twin for the online pyramid.  The scene is test_hip_ndt_pyramid.py's
(tests/ndt_pyramid_batch_reference.py holds its six start poses and three budgets); what the tests need of these inputs is
asserted from the single calls' results."""
import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_pyramid_batch_reference as B
from tests.helpers import CFG, net_from_params
from tests.test_hip_ndt_online_pyramid import make as make_online
from tests.test_hip_ndt_online_pyramid import raw_level
from tests.test_ndt_cpu import KW, LEAF, T_INIT, T_TRUE

pytestmark = pytest.mark.gpu

RESOLUTIONS = B.RESOLUTIONS
TOL_FLOOR = 1e-12      # this project's rule for float64 comparisons that differ only in the order of a sum
MIN_CORR = 50


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def map_xyz():
    return B.scene()["map_xyz"]


@pytest.fixture(scope="module")
def scan():
    return dev(B.scene()["scan"])


@pytest.fixture(scope="module")
def pyr(map_xyz):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(map_xyz, resolutions=RESOLUTIONS, leaf=LEAF, iterations=90, level_iterations=(30, 30, 30))


@pytest.fixture(scope="module")
def fine(map_xyz):
    """a plain localiser whose single map has the finest level's resolution"""
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(map_xyz, resolution=RESOLUTIONS[-1], leaf=LEAF)


@pytest.fixture(scope="module")
def points(pyr, scan):
    """the scan as the device thins it: (float64 [n, 3] on the device, n as a device int32), read-only"""
    res = pyr.submit(scan, len(scan), T_TRUE, iterations=0).result()
    assert res.n_points == len(B.scene()["pts"]) == 4157
    return pyr._pts[:res.n_points].clone(), torch.full((1,), res.n_points, dtype=torch.int32, device="cuda")


# ---- the C ABI itself --------------------------------------------------------------------------------------------------------
FILL = 7.25            # what every output holds before a call: a row the call never wrote would keep it


def raw_single(loc, pts, n_dev, T, iters, caps, min_corr=MIN_CORR, cap=None):
    from sps_amd import _native
    cap = len(pts) if cap is None else cap
    T_out = torch.full((16,), FILL, dtype=torch.float64, device="cuda")
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    trace = torch.full((max(iters, 1), 4), FILL, dtype=torch.float64, device="cuda")
    normal = torch.full((max(iters, 1), 28), FILL, dtype=torch.float64, device="cuda")
    level = torch.full((max(iters, 1),), 77, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(_native.lib.sps_ndt_pyramid_align_scratch(cap), dtype=torch.uint8, device="cuda")
    loc.ctx.ndt_pyramid_align(pts.data_ptr(), n_dev.data_ptr(), cap, T, iters, caps, loc.neighbours, min_corr, loc.tol_t, loc.tol_r,
                              T_out.data_ptr(), status.data_ptr(), trace.data_ptr() if iters else None,
                              normal.data_ptr() if iters else None, level.data_ptr() if iters else None, scratch.data_ptr(), stream())
    return dict(T_out=T_out.cpu().numpy(), status=status.cpu().numpy(), trace=trace.cpu().numpy()[:iters],
                normal=normal.cpu().numpy()[:iters], level=level.cpu().numpy()[:iters])


def raw_batch(loc, pts, n_dev, T_inits, iters, caps, min_corr=MIN_CORR, cap=None):
    """sps_ndt_pyramid_align_batch itself: every output as it lies in memory.  T_inits: a host array [K, 4, 4] or a device
    tensor of K * 16 float64"""
    from sps_amd import _native
    cap = len(pts) if cap is None else cap
    T_dev = T_inits if torch.is_tensor(T_inits) else dev(np.asarray(T_inits, dtype=np.float64))
    K = T_dev.numel() // 16
    I = max(iters, 1)
    T_out = torch.full((K, 16), FILL, dtype=torch.float64, device="cuda")
    status = torch.full((K, 4), 77, dtype=torch.int32, device="cuda")
    trace = torch.full((K, I, 4), FILL, dtype=torch.float64, device="cuda")
    normal = torch.full((K, I, 28), FILL, dtype=torch.float64, device="cuda")
    level = torch.full((K, I), 77, dtype=torch.int32, device="cuda")
    final = torch.full((K, 2), FILL, dtype=torch.float64, device="cuda")
    best = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    T_best = torch.full((16,), FILL, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(_native.lib.sps_ndt_pyramid_align_batch_scratch(cap, K), dtype=torch.uint8, device="cuda")
    loc.ctx.ndt_pyramid_align_batch(pts.data_ptr(), n_dev.data_ptr(), cap, T_dev.data_ptr(), K, iters, caps, loc.neighbours, min_corr,
                                    loc.tol_t, loc.tol_r, T_out.data_ptr(), status.data_ptr(), trace.data_ptr() if iters else None,
                                    normal.data_ptr() if iters else None, level.data_ptr() if iters else None, final.data_ptr(),
                                    best.data_ptr(), T_best.data_ptr(), scratch.data_ptr(), stream())
    loc.ctx.check_errors(stream())
    return dict(T_out=T_out.cpu().numpy(), status=status.cpu().numpy(), trace=trace.cpu().numpy()[:, :iters],
                normal=normal.cpu().numpy()[:, :iters], level=level.cpu().numpy()[:, :iters], final=final.cpu().numpy(),
                best=best.cpu().numpy(), T_best=T_best.cpu().numpy(), T_init=T_dev.cpu().numpy().reshape(K, 16))


def assert_hypothesis_is(got, k, one, what=""):
    for name in ("T_out", "status", "trace", "normal", "level"):
        a, b = got[name][k], one[name]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, name)


def assert_selection(got, min_corr=MIN_CORR):
    """best and T_best follow from status, final and the poses by k_ndt_select's rule (restated in the reference module)"""
    K = len(got["status"])
    counts = got["final"][:, 1].astype(np.int64)
    b = B.select(got["final"][:, 0], counts, got["status"][:, 0], min_corr)
    assert list(got["best"]) == B.best_words(b, got["status"][:, 0], counts, K)
    assert got["T_best"].tobytes() == (got["T_out"][b] if b >= 0 else got["T_init"][0]).tobytes()
    return b


@pytest.fixture(scope="module")
def singles(pyr, points):
    """sps_ndt_pyramid_align of every start at every budget, and that the inputs are what the tests need"""
    pts, n_dev = points
    out = []
    for budget, (caps, iters) in enumerate(B.BUDGETS):
        ones = [raw_single(pyr, pts, n_dev, T, iters, caps) for T in B.POSES]
        slots = [int(o["status"][1]) for o in ones]
        B.check_input_properties(budget, [int(o["status"][0]) for o in ones], slots, [o["level"][:s] for o, s in zip(ones, slots)],
                                 [o["T_out"].reshape(4, 4) for o in ones] if budget == 0 else None)
        for o, s in zip(ones, slots):                                          # slots that did no work: zero rows and level -1
            assert not o["trace"][s:].any() and not o["normal"][s:].any() and (o["level"][s:] == -1).all()
        out.append(ones)
    return out


# 1. hypothesis k is the single call
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 64])
@pytest.mark.parametrize("budget", [0, 1, 2])
def test_hypothesis_k_is_the_single_call(pyr, points, singles, budget, K):
    pts, n_dev = points
    caps, iters = B.BUDGETS[budget]
    # K < 6 counts down from the start off the map, so every K has a hypothesis that is final in slot 0
    idx = [k % 6 for k in range(K)] if K == 64 else [5 - k for k in range(K)]
    got = raw_batch(pyr, pts, n_dev, B.POSES[idx], iters, caps)
    for k, i in enumerate(idx):
        assert_hypothesis_is(got, k, singles[budget][i], (budget, K))
    assert got["T_out"][idx.index(B.OFF)].tobytes() == B.POSES[B.OFF].tobytes()   # status 2: the start pose, bit for bit
    b = assert_selection(got)
    assert (b == -1) == (K == 1) and got["best"][3] == K
    if K == 64:                                                                # the order changes no hypothesis' bytes
        rev = raw_batch(pyr, pts, n_dev, B.POSES[idx[::-1]], iters, caps)
        for k, i in enumerate(idx[::-1]):
            assert_hypothesis_is(rev, k, singles[budget][i], (budget, "reversed"))
            assert rev["final"][k].tobytes() == got["final"][63 - k].tobytes()
        assert rev["final"][assert_selection(rev)].tobytes() == got["final"][b].tobytes()   # and the same score wins


# 2. point counts around a workgroup of launch A, and the capacity
@pytest.mark.parametrize("n", [0, 31, 32, 33, 1000])
def test_point_counts(pyr, points, n):
    pts, _ = points
    cap = 1000
    buf = pts[:cap].clone()
    n_dev = torch.full((1,), len(pts) if n == cap else n, dtype=torch.int32, device="cuda")   # 1000: a count above the capacity
    ones = [raw_single(pyr, buf, n_dev, T, 6, (2, 2, 2), 10, cap) for T in B.POSES]
    got = raw_batch(pyr, buf, n_dev, B.POSES, 6, (2, 2, 2), 10, cap)
    for k, one in enumerate(ones):
        assert_hypothesis_is(got, k, one, n)
    assert_selection(got, 10)
    print(f"n {n}: status {list(got['status'][:, 0])} slots {list(got['status'][:, 1])} final counts {list(got['final'][:, 1])}")
    if n == 0:
        assert (got["status"] == [2, 1, 0, 0]).all() and list(got["best"]) == [-1, -1, 0, 6] and not got["final"].any()
        assert got["T_out"].tobytes() == got["T_init"].tobytes()
    else:
        assert got["final"][:, 1].max() <= min(n, cap) and (got["status"][:, 1] >= 1).all()


# 3. level counts
def test_one_level_is_the_single_map_batch(map_xyz, points):
    """every output has the bytes of sps_ndt_align_batch on a plain localiser of that resolution, a NaN start pose included"""
    from sps_amd import _native
    from sps_amd.localiser import NDTLocaliser
    pts, n_dev = points
    one = NDTLocaliser(map_xyz, resolutions=(1.0,), leaf=LEAF)
    plain = NDTLocaliser(map_xyz, resolution=1.0, leaf=LEAF)
    starts = np.concatenate([B.POSES, B.POSES[:1]])
    starts[6, 0, 3] = np.nan
    K, iters, cap = len(starts), 30, len(pts)
    got = raw_batch(one, pts, n_dev, starts, iters, (30,))
    T_dev = dev(starts)
    o = {name: torch.full(shape, 77 if dt == torch.int32 else FILL, dtype=dt, device="cuda") for name, shape, dt in (
        ("T_out", (K, 16), torch.float64), ("status", (K, 4), torch.int32), ("trace", (K, iters, 4), torch.float64),
        ("normal", (K, iters, 28), torch.float64), ("final", (K, 2), torch.float64), ("best", (4,), torch.int32),
        ("T_best", (16,), torch.float64))}
    scratch = torch.zeros(_native.lib.sps_ndt_align_batch_scratch(cap, K), dtype=torch.uint8, device="cuda")
    plain.ctx.ndt_align_batch(pts.data_ptr(), n_dev.data_ptr(), cap, T_dev.data_ptr(), K, iters, plain.neighbours, MIN_CORR,
                              plain.outlier_ratio, plain.tol_t, plain.tol_r, o["T_out"].data_ptr(), o["status"].data_ptr(),
                              o["trace"].data_ptr(), o["normal"].data_ptr(), o["final"].data_ptr(), o["best"].data_ptr(),
                              o["T_best"].data_ptr(), scratch.data_ptr(), stream())
    for name, t in o.items():
        assert got[name].tobytes() == t.cpu().numpy().tobytes(), name
    slots = got["status"][:, 1]
    assert all((got["level"][k, :s] == 0).all() and (got["level"][k, s:] == -1).all() for k, s in enumerate(slots))
    assert got["status"][6, 0] in (2, 3) and got["status"][B.OFF, 0] == 2 and got["status"][0, 0] == 0
    assert got["T_out"][6].tobytes() == starts[6].tobytes() and got["best"][0] not in (-1, 6, B.OFF)


@pytest.mark.parametrize("resolutions,caps", [((2.0, 1.0), (5, 30)), ((4.0, 2.0, 1.0, 0.5), (3, 4, 5, 30))])
def test_two_and_four_levels(map_xyz, points, resolutions, caps):
    from sps_amd.localiser import NDTLocaliser
    pts, n_dev = points
    loc = NDTLocaliser(map_xyz, resolutions=resolutions, leaf=LEAF)
    iters = 40
    ones = [raw_single(loc, pts, n_dev, T, iters, caps) for T in B.POSES]
    got = raw_batch(loc, pts, n_dev, B.POSES, iters, caps)
    for k, one in enumerate(ones):
        assert_hypothesis_is(got, k, one, resolutions)
    last = len(resolutions) - 1
    assert any(o["status"][3] == last and o["status"][0] == 0 for o in ones)   # the input: somebody converges on the last level
    assert len({int(o["status"][1]) for o in ones}) > 1                        # ... and they do not all take the same course
    assert_selection(got)


# 4. final scores
def test_final_scores_are_score_poses_on_the_finest_resolution(pyr, fine, points, scan):
    pts, n_dev = points
    for budget in (0, 2):                                                      # all reach the finest level; none does
        caps, iters = B.BUDGETS[budget]
        got = raw_batch(pyr, pts, n_dev, B.POSES, iters, caps)
        scores, counts = fine.score_poses(scan, len(scan), got["T_out"].reshape(-1, 4, 4)).result()
        assert got["final"][:, 0].tobytes() == scores.tobytes(), budget
        np.testing.assert_array_equal(got["final"][:, 1], counts)
    # iters = 0: the call is score_poses at the start poses
    got = raw_batch(pyr, pts, n_dev, B.POSES, 0, (30, 30, 30))
    scores, counts = fine.score_poses(scan, len(scan), B.POSES).result()
    assert got["final"][:, 0].tobytes() == scores.tobytes()
    np.testing.assert_array_equal(got["final"][:, 1], counts)
    assert got["T_out"].tobytes() == got["T_init"].tobytes() and (got["status"] == [1, 0, 0, 0]).all()
    assert counts[0] > 2500 and counts[B.OFF] == 0
    assert_selection(got)


# 5. selection
def test_selection(pyr, points, singles):
    pts, n_dev = points
    caps, iters = B.BUDGETS[0]
    got = raw_batch(pyr, pts, n_dev, B.POSES, iters, caps)
    b = assert_selection(got)
    # the 1.5 m start converged in the wrong basin with status 0; the score on the finest level tells
    assert got["status"][B.WRONG, 0] == 0 and b not in (B.WRONG, B.OFF, -1)
    assert LR.pose_difference(got["T_best"].reshape(4, 4), T_TRUE)[0] < 0.02
    assert abs(got["final"][0, 0] - 1583.93) < 0.01 and got["final"][B.WRONG, 0] < got["final"][0, 0] - 100.0
    print(f"final scores {list(got['final'][:, 0])}: best {b}")
    # two identical starts: the lower index
    got = raw_batch(pyr, pts, n_dev, np.stack([T_INIT, T_INIT, B.POSES[B.OFF]]), iters, caps)
    assert got["final"][0].tobytes() == got["final"][1].tobytes() and list(got["best"][[0, 3]]) == [0, 3]
    assert_selection(got)
    # nobody qualifies
    off = B.POSES[[B.OFF] * 3].copy()
    off[1, 1, 3] += 1.0
    got = raw_batch(pyr, pts, n_dev, off, iters, caps)
    assert list(got["best"]) == [-1, -1, 0, 3] and got["T_best"].tobytes() == off[0].tobytes()
    # four slots: the selected hypothesis never reached the finest level
    caps, iters = B.BUDGETS[2]
    got = raw_batch(pyr, pts, n_dev, B.POSES, iters, caps)
    b = assert_selection(got)
    assert b >= 0 and got["status"][b, 0] == 1 and got["status"][b, 3] == 1 and 2 not in got["level"][b]


# 6. Python
def same_result(r, got, k):
    """PoseResult r against hypothesis k of the raw outputs"""
    code, it, n_corr, _ = (int(v) for v in got["status"][k])
    assert (r.status, r.iterations, r.n_corr) == (code, it, n_corr)
    assert r.pose.tobytes() == got["T_out"][k].tobytes() and r.trace.tobytes() == got["trace"][k, :it].tobytes()
    assert r.normal.tobytes() == got["normal"][k, :it].tobytes()
    np.testing.assert_array_equal(r.levels, got["level"][k, :it])
    assert len(r.levels) == it


def same_batch_result(res, got):
    for k, r in enumerate(res.results):
        same_result(r, got, k)
    assert res.scores.tobytes() == got["final"][:, 0].tobytes()
    np.testing.assert_array_equal(res.counts, got["final"][:, 1])
    assert res.best == got["best"][0] and res.pose.tobytes() == got["T_best"].tobytes()


def test_submit_batch_parses_to_the_raw_call(pyr, points, scan):
    pts, n_dev = points
    got = raw_batch(pyr, pts, n_dev, B.POSES, 90, (30, 30, 30))
    res = pyr.submit_batch(scan, len(scan), B.POSES, with_normal=True, coarse_to_fine=True).result()
    assert len(res.results) == 6 and res.results[0].n_points == len(pts) and res.map_update is None and res.map_carve is None
    same_batch_result(res, got)
    short = pyr.submit_batch(scan, len(scan), B.POSES[:2], iterations=4, coarse_to_fine=True).result()   # caps: (30, 30, 30)
    assert [list(r.levels) for r in short.results] == [[0, 0, 0, 0]] * 2 and short.results[0].normal is None
    zero = pyr.submit_batch(scan, len(scan), B.POSES[:2], iterations=0, coarse_to_fine=True).result()
    assert [len(r.levels) for r in zero.results] == [0, 0] and zero.best == 0


def test_submit_from_device_equals_submit_on_the_pyramid(pyr, scan):
    src = dev(B.POSES[1])
    T_dev = torch.zeros(16, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        T_dev.copy_(src.reshape(-1))                                           # the kernel that writes the pose, queued in front
        pend = pyr.submit_from_device(scan, len(scan), T_dev, with_normal=True, coarse_to_fine=True)
    b = pend.result()
    a = pyr.submit(scan, len(scan), B.POSES[1], with_normal=True).result()
    r = b.results[0]
    assert b.best == 0 and a.status == 0 and len(set(a.levels)) == 3
    assert (a.status, a.iterations, a.n_corr, a.n_points) == (r.status, r.iterations, r.n_corr, r.n_points)
    for x, y in ((a.pose, r.pose), (a.pose, b.pose), (a.trace, r.trace), (a.normal, r.normal), (a.levels, r.levels)):
        assert x.tobytes() == y.tobytes()
    o = pend._layout()
    words = pend._host.numpy()[o["status"]:o["n_points"]].view(np.int32)
    assert list(words) == [a.status, a.iterations, a.n_corr, 2]


def test_relocalise_is_score_top_and_the_batch(pyr, points, scan):
    from sps_amd.localiser import pose_grid
    pts, n_dev = points
    grid = B.POSES[1] @ pose_grid((-1.0, -0.5, 0.0, 0.5), (0.0, 0.5), (0.0, 4.0))
    P, K = len(grid), 5
    res = pyr.relocalise(scan, len(scan), grid, keep=K, with_normal=True, iterations=40, coarse_to_fine=True).result()
    # by hand: the scores on the single map, the best K of them, the batch from those poses on the pyramid
    sp = pyr.score_poses(scan, len(scan), grid)
    scores, counts = sp.result()
    top = torch.full((K,), -7, dtype=torch.int32, device="cuda")
    T_top = torch.zeros(K * 16, dtype=torch.float64, device="cuda")
    n_top = torch.zeros(1, dtype=torch.int32, device="cuda")
    pyr.ctx.ndt_top_poses(sp._keep[2].data_ptr(), sp._keep[4].data_ptr(), P, pyr.min_correspondences, K, top.data_ptr(),
                          T_top.data_ptr(), n_top.data_ptr(), stream())
    got = raw_batch(pyr, pts, n_dev, T_top, 40, (30, 30, 30))
    assert res.scores.tobytes() == scores.tobytes() and np.array_equal(res.counts, counts)
    np.testing.assert_array_equal(res.candidates, top.cpu().numpy())
    assert int(n_top.item()) == K and len(set(res.candidates)) == K
    same_batch_result(res.batch, got)
    assert res.index == res.candidates[res.batch.best] and res.ok and res.pose.tobytes() == got["T_best"].tobytes()


def test_without_the_argument_nothing_changes(pyr, scan):
    from sps_amd.localiser import pose_grid
    grid = B.POSES[2] @ pose_grid((0.0, 0.5), (0.0,), (0.0, 4.0))
    T_dev = dev(B.POSES[2])
    for call in (lambda **kw: pyr.submit_batch(scan, len(scan), B.POSES, with_normal=True, iterations=8, **kw),
                 lambda **kw: pyr.submit_from_device(scan, len(scan), T_dev, iterations=8, **kw),
                 lambda **kw: pyr.relocalise(scan, len(scan), grid, keep=2, iterations=8, **kw)):
        a, b = call(), call(coarse_to_fine=False)
        ra, rb = a.result(), b.result()
        assert a._host.numpy().tobytes() == b._host.numpy().tobytes()
        first = (ra.batch if hasattr(ra, "batch") else ra).results[0]
        assert first.levels is None and first.iterations > 1


# 7. the online pyramid
CARVE = dict(min_pass=1, miss_frames=1)        # one frame clears: the carve leaves a trace in the maps


def levels_of(loc):
    return [(raw_level(loc, l), loc.carve_state(l), loc.pyramid_info(l)) for l in range(len(loc.resolutions))]


def assert_same_levels(a, b, what=""):
    for l, ((ca, sa, ia), (cb, sb, ib)) in enumerate(zip(a, b)):
        for name in ca:
            assert ca[name].tobytes() == cb[name].tobytes(), (what, l, name)
        for x, y in zip(sa, sb):
            assert x.tobytes() == y.tobytes(), (what, l, "carve state")
        assert ia == ib, (what, l)


def test_the_online_pyramid_is_updated_and_carved_at_the_selected_pose(map_xyz, scan):
    loc, twin = make_online(map_xyz), make_online(map_xyz)
    fresh = levels_of(loc)
    starts = B.POSES[[B.OFF, B.WRONG, 2]]
    res = loc.submit_batch(scan, len(scan), starts, coarse_to_fine=True, integrate=True, carve=True, carve_options=CARVE).result()
    one = twin.submit(scan, len(scan), starts[res.best], integrate=True, carve=True, carve_options=CARVE).result()
    assert res.best == 2 and one.status in (0, 1) and one.pose.tobytes() == res.pose.tobytes()
    assert isinstance(res.map_update, tuple) and len(res.map_update) == 3 and res.map_update == one.map_update
    assert isinstance(res.map_carve, tuple) and len(res.map_carve) == 3 and res.map_carve == one.map_carve
    assert all(u.points > 0 for u in res.map_update) and all(c.rays > 0 for c in res.map_carve)
    after = levels_of(loc)
    assert_same_levels(after, levels_of(twin), "selected")
    assert any(a[0]["count"].tobytes() != f[0]["count"].tobytes() for a, f in zip(after, fresh))   # ... and something happened
    # nobody selected: no byte of any level moves
    off = B.POSES[[B.OFF] * 2]
    res = loc.submit_batch(scan, len(scan), off, coarse_to_fine=True, integrate=True, carve=True, carve_options=CARVE).result()
    assert res.best == -1 and res.pose.tobytes() == off[0].tobytes()
    assert [(u.founded, u.dropped, u.points) for u in res.map_update] == [(0, 0, 0)] * 3
    assert [u.cells for u in res.map_update] == [i[2][0] for i in after]
    assert [(c.rays, c.seen_through, c.cleared, c.cut) for c in res.map_carve] == [(0, 0, 0, 0)] * 3
    assert_same_levels(levels_of(loc), after, "nobody selected")
    # the search takes the same road
    from sps_amd.localiser import pose_grid
    rel = loc.relocalise(scan, len(scan), T_INIT @ pose_grid((0.0, 0.5), (0.0,), (0.0,)), keep=2, coarse_to_fine=True, integrate=True,
                         carve=True).result()
    assert rel.ok and len(rel.map_update) == 3 and len(rel.map_carve) == 3 and rel.map_update[2].points > 0
    loc.ctx.check_errors(stream())


# 8. the loop
@pytest.fixture(scope="module")
def sequence():
    """three frames of the synthetic sequence of the driver's --synthetic replay: 0.5 m per scan along x"""
    n, step = 3, 0.5
    mp = synthetic.sequence_map(n, step, **KW)
    truth, scans = [], []
    for i in range(n):
        world = synthetic.lidar_scan(100 + i, x_offset=step * i, **KW)
        T = LR.perturbation(step * i, 0.0, 0.0, 0.0)
        scans.append(np.c_[world[:, :3].astype(np.float64) - T[:3, 3], world[:, 3]].astype(np.float32))
        truth.append(T)
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    return mp, truth, scans, net, synthetic.sequence_imu(n, step=step, scan_period=0.1, rate=100.0)


def cvm_filter(net, mp):
    from sps_amd.sps_filters import SPSCVMFilter
    mpt = torch.from_numpy(np.ascontiguousarray(mp[:, :3], dtype=np.float32))
    return SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0)


def test_the_loop_takes_the_device_path_with_a_pyramid(sequence):
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser
    from sps_amd.pose_estimator import PoseEstimator
    mp, truth, scans, net, imu = sequence
    ndt = NDTLocaliser(mp[:, :3].astype(np.float64), resolutions=RESOLUTIONS, leaf=LEAF, iterations=30, level_iterations=(10, 10, 10))

    def run(device_guess):
        est = PoseEstimator(truth[0], "cuda", initial_velocity=(5.0, 0.0, 0.0))
        loop = LocalisationLoop(cvm_filter(net, mp), ndt, truth[0], estimator=est, device_guess=device_guess, coarse_to_fine=True)
        steps = [loop.step(s, imu=imu[k]) for k, s in enumerate(scans)]
        return loop, steps, est.state()

    dloop, on_dev, sd = run(None)
    hloop, on_host, sh = run(False)
    assert dloop.device_guess is True and hloop.device_guess is False
    for k, (a, b) in enumerate(zip(on_dev, on_host)):
        p, q = a.pose_result, b.pose_result
        print(f"frame {k}: status {p.status}/{q.status} slots {p.iterations}/{q.iterations} levels "
              f"{np.bincount(p.levels, minlength=3)} pose error {np.linalg.norm(a.pose[:3, 3] - truth[k][:3, 3]):.4f} m")
        assert not a.flagged and not b.flagged and a.batch is not None and b.batch is None, k
        assert a.guess.tobytes() == b.guess.tobytes() and a.pose.tobytes() == b.pose.tobytes(), k
        assert a.estimate.tobytes() == b.estimate.tobytes(), k
        assert (p.status, p.iterations, p.n_corr, p.n_points) == (q.status, q.iterations, q.n_corr, q.n_points), k
        assert p.trace.tobytes() == q.trace.tobytes() and p.levels.tobytes() == q.levels.tobytes() and len(set(p.levels)) == 3, k
    for x, y in ((sd.mean, sh.mean), (sd.covariance, sh.covariance), (sd.pose, sh.pose)):
        assert x.tobytes() == y.tobytes()
    assert (sd.n_predict, sd.n_correct) == (sh.n_predict, sh.n_correct) and sd.n_correct == 3 and sd.n_predict > 0
    with pytest.raises(ValueError):                                            # without the argument the pyramid has no device path
        LocalisationLoop(type("TakesNone", (), dict(takes_pose=False))(), ndt, truth[0], estimator=PoseEstimator(truth[0], "cuda"),
                         device_guess=True)


def test_the_loop_with_hypotheses_on_an_online_pyramid(sequence):
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser, pose_grid
    from sps_amd.pose_estimator import PoseEstimator
    mp, truth, scans, net, imu = sequence
    xyz = mp[:, :3].astype(np.float64)
    caps = tuple(max(2 * len(np.unique(np.floor(xyz / r).astype(np.int64), axis=0)), 4096) for r in RESOLUTIONS)
    ndt = NDTLocaliser(xyz, resolutions=RESOLUTIONS, leaf=LEAF, iterations=30, level_iterations=(10, 10, 10), level_capacities=caps)
    est = PoseEstimator(truth[0], "cuda", initial_velocity=(5.0, 0.0, 0.0))
    loop = LocalisationLoop(cvm_filter(net, mp), ndt, truth[0], hypotheses=pose_grid((0.0, 0.5), (0.0,), (0.0,)), update_map=True,
                            carve_map=True, estimator=est, coarse_to_fine=True)
    assert loop.device_guess is False
    for k, s in enumerate(scans):
        st = loop.step(s, imu=imu[k])
        b = st.batch
        assert not st.flagged and b.best >= 0 and len(b.results) == 2 and all(r.levels is not None for r in b.results)
        assert isinstance(b.map_update, tuple) and len(b.map_update) == 3 and all(u.points > 0 for u in b.map_update), k
        assert isinstance(b.map_carve, tuple) and len(b.map_carve) == 3 and all(c.rays > 0 for c in b.map_carve), k
        assert np.linalg.norm(st.pose[:3, 3] - truth[k][:3, 3]) < 0.1, k
    ndt.ctx.check_errors(stream())


# 9. refusals, all before any device work
def test_refusals(pyr, fine, points, scan, map_xyz):
    from sps_amd import _native
    from sps_amd.localiser import NDTLocaliser
    pts, n_dev = points
    T_dev = dev(T_INIT)
    for loc in (fine, NDTLocaliser(map_xyz[:4000], source="cells", capacity=1000)):
        with pytest.raises(ValueError):
            loc.submit_batch(scan, len(scan), B.POSES, coarse_to_fine=True)
        with pytest.raises(ValueError):
            loc.submit_from_device(scan, len(scan), T_dev, coarse_to_fine=True)
        with pytest.raises(ValueError):
            loc.relocalise(scan, len(scan), B.POSES, coarse_to_fine=True)
    with pytest.raises(ValueError):
        pyr.submit_batch(scan, len(scan), np.tile(np.eye(4), (65, 1, 1)), coarse_to_fine=True)
    with pytest.raises(ValueError):
        pyr.submit_batch(scan, len(scan), np.zeros((0, 4, 4)), coarse_to_fine=True)
    with pytest.raises(ValueError):
        pyr.relocalise(scan, len(scan), B.POSES, keep=65, coarse_to_fine=True)
    with pytest.raises(ValueError):                                            # a static pyramid has no map to integrate into
        pyr.submit_batch(scan, len(scan), B.POSES, coarse_to_fine=True, integrate=True)
    lib = _native.lib
    assert lib.sps_ndt_pyramid_align_batch_scratch(len(pts), 0) == lib.sps_ndt_pyramid_align_batch_scratch(len(pts), 65) == -1
    for K in (0, 65):                                                          # refused before anything is launched or read
        with pytest.raises(_native.SpsError, match="n_hyp"):
            pyr.ctx.ndt_pyramid_align_batch(pts.data_ptr(), n_dev.data_ptr(), len(pts), T_dev.data_ptr(), K, 2, (30, 30, 30), 7, 50,
                                            1e-4, 1e-5, *([T_dev.data_ptr()] * 9), stream())
    for caps, neighbours in (((30, 30, 0), 7), ((30, 30, 30), 5)):             # bad level_iters; neighbours as the single call checks
        with pytest.raises(_native.SpsError):
            pyr.ctx.ndt_pyramid_align_batch(pts.data_ptr(), n_dev.data_ptr(), len(pts), T_dev.data_ptr(), 1, 2, caps, neighbours, 50,
                                            1e-4, 1e-5, *([T_dev.data_ptr()] * 9), stream())
    with pytest.raises(_native.SpsError, match="sps_ndt_pyramid_build has not been called"):   # the single map is no pyramid
        fine.ctx.ndt_pyramid_align_batch(pts.data_ptr(), n_dev.data_ptr(), len(pts), T_dev.data_ptr(), 1, 2, (30,), 7, 50, 1e-4, 1e-5,
                                         *([T_dev.data_ptr()] * 9), stream())
    pyr.ctx.check_errors(stream())


# ---- against the restatement ---------------------------------------------------------------------------------------------------
def test_the_batch_matches_the_restatement(pyr, points):
    """Status, slots, levels and the count of every slot exactly; poses within 100 x the restatement's own forward-versus-
    reversed spread on that hypothesis, floored at 1e-12 (this project's rule); the points counted on the finest level and
    the selection exactly."""
    pts, n_dev = points
    budget = 1
    caps, iters = B.BUDGETS[budget]
    fwd, rev = B.restated(budget), B.restated(budget, True)
    got = raw_batch(pyr, pts, n_dev, B.POSES, iters, caps)
    for k, (f, r) in enumerate(zip(fwd["results"], rev["results"])):
        st, sr = LR.pose_difference(f["pose"], r["pose"])
        tol_t, tol_r = max(100.0 * st, TOL_FLOOR), max(100.0 * sr, TOL_FLOOR)
        dt, dr = LR.pose_difference(got["T_out"][k].reshape(4, 4), f["pose"])
        print(f"{B.NAMES[k]:12s}: status {got['status'][k, 0]}/{f['status']} slots {got['status'][k, 1]}/{f['iterations']} spread "
              f"{st:.3e} m {sr:.3e} rad device vs restatement {dt:.3e} m {dr:.3e} rad")
        assert f["faces"] == 0 and f["boundary"] == 0
        assert list(got["status"][k]) == [f["status"], f["iterations"], f["n_corr"], f["level"]], k
        s = f["iterations"]
        np.testing.assert_array_equal(got["level"][k, :s], f["levels"])
        np.testing.assert_array_equal(got["trace"][k, :s, 0], f["trace"][:, 0])
        assert dt <= tol_t and dr <= tol_r, k
    np.testing.assert_array_equal(got["final"][:, 1], fwd["counts"])
    assert got["best"][0] == fwd["best"]
