"""GPU tests of distribution-to-distribution NDT from several poses (sps_ndt_align_d2d_batch, sps_ndt_score_poses_d2d and
the ``d2d=True`` calls of NDTLocaliser(source="cells"); C ABI: the "NDT localiser, distribution to distribution, several
poses" section of include/sps_hip.h): device against device bit for bit, the raw calls at their edges, and
the device against the numpy restatement in tests/ndt_d2d_batch_reference.py.  The scene is that of test_hip_ndt_d2d.py
at leaf 0.4: 4 157 thinned points, 246 valid source cells among 1 226 records."""
import math

import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_batch_reference as NB
from tests import ndt_d2d_batch_reference as DBR
from tests import ndt_d2d_reference as DR
from tests import ndt_reference as NR
from tests.helpers import CFG, net_from_params
from tests.test_ndt_d2d_batch_cpu import CENTRE, LEAF, scene_d2d
from tests.test_ndt_d2d_cpu import KW, T_INIT, T_TRUE, sensor_scan

pytestmark = pytest.mark.gpu

RES = 1.0
TOL_FLOOR = 1e-12      # this project's rule for float64 comparisons that differ only in the order of a sum
TILE = 32              # NDT_SCORE_TILE
OLD_TEXT = "registers points: it needs an NDTLocaliser with source='points'"


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def scene():
    return scene_d2d()


@pytest.fixture(scope="module")
def scan(scene):
    return dev(scene["scan"])


@pytest.fixture(scope="module")
def loc(scene):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF, source="cells")


@pytest.fixture(scope="module")
def loc1(scene):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF, source="cells", neighbours=1)


@pytest.fixture(scope="module")
def batch18(loc, scene, scan):
    """the 18-hypothesis batch on the device, computed once"""
    return loc.submit_batch(scan, len(scan), scene["starts"], with_normal=True, d2d=True).result()


@pytest.fixture(scope="module")
def grid_scores(loc, scene, scan):
    """the scores of the 45-pose grid on the device, computed once"""
    return loc.score_poses(scan, len(scan), scene["grid"], d2d=True).result()


@pytest.fixture(scope="module")
def tol(scene):
    """the pose tolerance of test_hip_ndt_batch.py, for this registration: 100 x the restatement's forward / reversed
    spread, floored at 1e-12"""
    spread_t, spread_r = LR.pose_difference(scene["ref"]["results"][CENTRE]["pose"], scene["rev"]["pose"])
    t = max(100.0 * spread_t, TOL_FLOOR), max(100.0 * spread_r, TOL_FLOOR)
    print(f"spread forward/reversed: {spread_t:.3e} m {spread_r:.3e} rad -> tolerance {t[0]:.3e} m {t[1]:.3e} rad")
    return t


def same_bits(a, b):
    assert (a.status, a.iterations, a.n_corr, a.n_points, a.n_sources) == (b.status, b.iterations, b.n_corr, b.n_points, b.n_sources)
    for x, y in ((a.pose, b.pose), (a.trace, b.trace), (a.normal, b.normal)):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()


def same_batch(a, b):
    assert len(a.results) == len(b.results) and a.best == b.best
    for x, y in zip(a.results, b.results):
        same_bits(x, y)
    assert a.scores.tobytes() == b.scores.tobytes() and a.counts.tobytes() == b.counts.tobytes()
    assert a.pose.tobytes() == b.pose.tobytes()


# ---- the raw calls -----------------------------------------------------------------------------------------------------------
def upload(rec, n_src, cap):
    """records for a raw call: a buffer of max(len(rec), cap, 1) + 1 rows, and (n_src, 0) on the device"""
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, 10)
    buf = np.zeros((max(len(rec), cap, 1) + 1, 10))
    buf[:len(rec)] = rec
    return dev(buf), torch.tensor([n_src, 0], dtype=torch.int32, device="cuda")


def raw_score(loc, rec, poses, n_src=None, cap=None, neighbours=7, uploaded=None):
    """sps_ndt_score_poses_d2d itself on hand-uploaded records: (scores [P], counts [P])"""
    from sps_amd import _native
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, 10)
    cap = len(rec) if cap is None else cap
    r, n = uploaded if uploaded is not None else upload(rec, len(rec) if n_src is None else n_src, cap)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    P = len(poses)
    T = dev(poses)
    out = torch.full((P, 2), -7.5, dtype=torch.float64, device="cuda")
    scratch = torch.empty(_native.lib.sps_ndt_score_d2d_scratch(cap, P), dtype=torch.uint8, device="cuda")
    loc.ctx.ndt_score_poses_d2d(r.data_ptr(), n.data_ptr(), cap, T.data_ptr(), P, neighbours, 0.55, out.data_ptr(), scratch.data_ptr(),
                                stream())
    h = out.cpu().numpy()
    loc.ctx.check_errors(stream())
    return h[:, 0].copy(), h[:, 1].copy()


def raw_batch(loc, rec, T_inits, n_src=None, cap=None, iters=30, neighbours=7, min_corr=50):
    """sps_ndt_align_d2d_batch itself: dict(pose [K, 4, 4], status [K, 4], trace, normal, final [K, 2], best [4], T_best)"""
    from sps_amd import _native
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, 10)
    cap = len(rec) if cap is None else cap
    r, n = upload(rec, len(rec) if n_src is None else n_src, cap)
    T_inits = np.ascontiguousarray(T_inits, dtype=np.float64).reshape(-1, 4, 4)
    K, I = len(T_inits), iters
    T = dev(T_inits)
    at = np.cumsum([0, 16 * K, 2 * K, 4 * K * I, 28 * K * I, 2 * K, 2, 16])
    out = torch.full((int(at[-1]),), -7.5, dtype=torch.float64, device="cuda")
    p = [out.data_ptr() + int(a) * 8 for a in at]
    scratch = torch.empty(_native.lib.sps_ndt_align_d2d_batch_scratch(cap, K), dtype=torch.uint8, device="cuda")
    loc.ctx.ndt_align_d2d_batch(r.data_ptr(), n.data_ptr(), cap, T.data_ptr(), K, I, neighbours, min_corr, 0.55, 1e-4, 1e-5, p[0], p[1],
                                p[2] if I else None, p[3] if I else None, p[4], p[5], p[6], scratch.data_ptr(), stream())
    h = out.cpu().numpy()
    loc.ctx.check_errors(stream())
    return dict(pose=h[at[0]:at[1]].reshape(K, 4, 4), status=h[at[1]:at[2]].view(np.int32).reshape(K, 4),
                trace=h[at[2]:at[3]].reshape(K, I, 4), normal=h[at[3]:at[4]].reshape(K, I, 28), final=h[at[4]:at[5]].reshape(K, 2),
                best=h[at[5]:at[6]].view(np.int32), T_best=h[at[6]:at[7]].reshape(4, 4))


def from_first_valid(scene):
    """the scene's records from its first valid one on: record 0 is valid, invalid ones follow in between"""
    rec = DR.records(scene["src"])
    return rec[int(np.argmax(rec[:, 9] != 0.0)):]


# ---- 1. device against device, bit for bit -------------------------------------------------------------------------------------
def starts_for(scene, n_hyp):
    if n_hyp == 1:
        return scene["starts"][[CENTRE]]
    if n_hyp <= 18:
        return scene["starts"][:n_hyp]
    g = NB.grid(np.linspace(-1.75, 1.75, 8), (-1.0, -0.35, 0.35, 1.0), (0.0, 8.0))
    assert len(g) == n_hyp == 64
    return np.stack([T_INIT @ d for d in g])


@pytest.mark.parametrize("neighbours,n_hyp", [(7, 18), (1, 18), (7, 1), (7, 64)])
def test_batch_equals_single_calls(loc, loc1, scene, scan, neighbours, n_hyp):
    L = loc if neighbours == 7 else loc1
    starts = starts_for(scene, n_hyp)
    got = L.submit_batch(scan, len(scan), starts, with_normal=True, d2d=True).result()
    assert len(got.results) == n_hyp and got.scores.shape == (n_hyp,) and got.counts.shape == (n_hyp,)
    ran = set()
    for k in range(n_hyp):
        one = L.submit(scan, len(scan), starts[k], with_normal=True).result()
        same_bits(got.results[k], one)
        assert got.results[k].normal is not None and one.iterations >= 1 and one.n_sources == scene["src"]["n_src"][1]
        ran.add((one.status, one.iterations))
    assert n_hyp == 1 or len(ran) > 1          # the hypotheses did not all take the same course
    assert got.pose.tobytes() == (got.results[got.best].pose if got.best >= 0 else starts[0]).tobytes()
    L.ctx.check_errors(stream())


def test_score_poses_equals_the_zero_iteration_batch(loc, scene, scan, grid_scores):
    sc, cnt = grid_scores
    zero = loc.submit_batch(scan, len(scan), scene["grid"], iterations=0, d2d=True).result()
    assert zero.scores.tobytes() == sc.tobytes() and zero.counts.tobytes() == cnt.tobytes()
    assert [(r.status, r.iterations) for r in zero.results] == [(1, 0)] * len(sc)
    assert all(r.pose.tobytes() == g.tobytes() for r, g in zip(zero.results, scene["grid"]))
    assert len(set(sc.tolist())) == len(sc) and cnt.min() >= loc.min_correspondences
    loc.ctx.check_errors(stream())


def test_relocalise_is_score_top_and_the_batch(loc, scene, scan, grid_scores):
    K = 4
    rel = loc.relocalise(scan, len(scan), scene["grid"], keep=K, with_normal=True, d2d=True).result()
    sc, cnt = grid_scores
    assert rel.scores.tobytes() == sc.tobytes() and rel.counts.tobytes() == cnt.tobytes()
    P = len(sc)
    score_dev, T_dev = dev(np.stack([sc, cnt.astype(np.float64)], axis=1)), dev(scene["grid"])
    top = torch.full((K,), -7, dtype=torch.int32, device="cuda")
    T_top = torch.zeros((K, 4, 4), dtype=torch.float64, device="cuda")
    n_top = torch.zeros(1, dtype=torch.int32, device="cuda")
    loc.ctx.ndt_top_poses(score_dev.data_ptr(), T_dev.data_ptr(), P, loc.min_correspondences, K, top.data_ptr(), T_top.data_ptr(),
                          n_top.data_ptr(), stream())
    idx = top.cpu().numpy()
    assert list(rel.candidates) == list(idx) and int(n_top.item()) == K and (idx >= 0).all()
    batch = loc.submit_batch(scan, len(scan), T_top.cpu().numpy(), with_normal=True, d2d=True).result()
    same_batch(rel.batch, batch)
    assert rel.index == idx[batch.best] and rel.pose.tobytes() == batch.pose.tobytes() and rel.ok
    loc.ctx.check_errors(stream())


def test_submit_from_device_equals_submit(loc, scene, scan):
    for T in (T_INIT, scene["starts"][0]):
        a = loc.submit(scan, len(scan), T, with_normal=True).result()
        b = loc.submit_from_device(scan, len(scan), dev(T.reshape(16)), with_normal=True, d2d=True).result()
        assert len(b.results) == 1 and b.best == (0 if a.status in (0, 1) else -1)
        same_bits(a, b.results[0])
        assert b.pose.tobytes() == a.pose.tobytes()
    with pytest.raises(TypeError):
        loc.submit_from_device(scan, len(scan), T_INIT, d2d=True)               # a host array
    loc.ctx.check_errors(stream())


def test_two_calls_give_the_same_bits(loc, scene, scan, batch18, grid_scores):
    same_batch(batch18, loc.submit_batch(scan, len(scan), scene["starts"], with_normal=True, d2d=True).result())
    sc, cnt = loc.score_poses(scan, len(scan), scene["grid"], d2d=True).result()
    assert sc.tobytes() == grid_scores[0].tobytes() and cnt.tobytes() == grid_scores[1].tobytes()


def test_a_call_behind_a_kernel_on_a_side_stream_sees_its_data(loc, scene, scan):
    """the rows and the start pose are written on the side stream, behind a long product, right before the calls"""
    want = loc.submit(scan, len(scan), T_INIT, with_normal=True).result()
    want_sc = loc.score_poses(scan, len(scan), scene["grid"][:5], d2d=True).result()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    src_T = dev(T_INIT.reshape(16))
    with torch.cuda.stream(side):
        big = torch.ones((2048, 2048), device="cuda")
        for _ in range(8):
            big = (big @ big) * 1e-4
        rows = torch.zeros_like(scan)
        T_dev = torch.zeros(16, dtype=torch.float64, device="cuda")
        rows.copy_(scan)
        T_dev.copy_(src_T)
        pend = loc.submit_from_device(rows, len(scan), T_dev, with_normal=True, d2d=True)
        pend_sc = loc.score_poses(rows, len(scan), scene["grid"][:5], d2d=True)
    got, got_sc = pend.result(), pend_sc.result()
    same_bits(want, got.results[0])
    assert got_sc[0].tobytes() == want_sc[0].tobytes() and got_sc[1].tobytes() == want_sc[1].tobytes()
    side.synchronize()
    loc.ctx.check_errors(stream())


# ---- 2. the raw calls at their edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src,cap", [(0, 8), (1, 1), (1, 40), (32, 32), (32, 64), (33, 32), (33, 33), (33, 70), (100, 33)])
@pytest.mark.parametrize("P", [1, TILE + 1])
def test_edge_shapes_of_the_scorer_and_the_batch(loc, scene, n_src, cap, P):
    """the first min(n_src, cap) records count, whatever the capacity; the scorer, the zero-iteration batch and a call with
    the capacity cut to the records agree bit for bit; the restatement within the bound of section 3"""
    rec = from_first_valid(scene)[:max(n_src, 1)]
    m = min(n_src, cap)
    if m >= 32:
        assert 0 < int((rec[:m, 9] != 0.0).sum()) < m                          # invalid records interleaved with valid ones
    poses = np.concatenate([scene["grid"], scene["starts"]])[:P]
    sc, cnt = raw_score(loc, rec, poses, n_src=n_src, cap=cap)
    tight = raw_score(loc, rec[:m], poses, n_src=m, cap=m)
    assert sc.tobytes() == tight[0].tobytes() and cnt.tobytes() == tight[1].tobytes()
    for p0 in range(0, P, 64):
        b = raw_batch(loc, rec, poses[p0:p0 + 64], n_src=n_src, cap=cap, iters=0, min_corr=1)
        assert b["final"][:, 0].tobytes() == sc[p0:p0 + 64].tobytes() and b["final"][:, 1].tobytes() == cnt[p0:p0 + 64].tobytes()
        assert (b["status"] == [1, 0, 0, 0]).all() and b["pose"].tobytes() == poses[p0:p0 + 64].tobytes()
        qualify = [k for k in range(len(b["final"])) if b["final"][k, 1] >= 1]
        want = max(qualify, key=lambda k: (b["final"][k, 0], -k)) if qualify else -1
        assert b["best"][0] == want and b["best"][3] == len(b["final"])
        assert b["T_best"].tobytes() == poses[p0 + max(want, 0)].tobytes()
    sub = DR.hand_sources(rec[:m, :3], rec[:m, 3:9], rec[:m, 9] != 0.0)
    ref = DBR.score_poses(sub, scene["cmap"], poses)
    assert (ref["faces"] == 0).all() and (ref["boundary"] == 0).all()
    np.testing.assert_array_equal(cnt, ref["counts"])
    assert (np.abs(sc - ref["scores"]) <= (ref["m"] + 6) * 2.0 ** -52 * ref["sum_abs"]).all()
    if m == 0:
        assert (sc == 0.0).all() and (cnt == 0.0).all()
    elif m >= 32:
        assert cnt.min() >= 1 and (sc != 0.0).all()


def test_all_records_invalid(loc, scene):
    rec = from_first_valid(scene)[:70].copy()
    rec[:, 9] = 0.0
    sc, cnt = raw_score(loc, rec, scene["grid"][:TILE + 1])
    assert (sc == 0.0).all() and (cnt == 0.0).all()
    b = raw_batch(loc, rec, scene["starts"][:3])
    assert (b["status"][:, :3] == [2, 1, 0]).all() and list(b["best"]) == [-1, -1, 0, 3]
    assert b["pose"].tobytes() == scene["starts"][:3].tobytes() and b["T_best"].tobytes() == scene["starts"][0].tobytes()
    assert (b["final"] == 0.0).all()


def test_a_nan_pose_and_an_off_map_pose_leave_their_neighbours_alone(loc, scene, grid_scores):
    rec = DR.records(scene["src"])
    poses = scene["grid"][:5].copy()
    poses[1, 1, 2], poses[3, 0, 3] = np.nan, poses[3, 0, 3] + 5000.0
    sc, cnt = raw_score(loc, rec, poses)
    assert list(sc[[1, 3]]) == [0.0, 0.0] and list(cnt[[1, 3]]) == [0.0, 0.0]
    for k in (0, 2, 4):
        assert sc[k] == grid_scores[0][k] and cnt[k] == grid_scores[1][k]
    starts = scene["starts"][:5].copy()
    starts[1, 1, 2], starts[3, 0, 3] = np.nan, starts[3, 0, 3] + 5000.0
    b = raw_batch(loc, rec, starts)
    clean = raw_batch(loc, rec, scene["starts"][:5])
    assert list(b["status"][[1, 3], 0]) == [2, 2] and b["pose"][3].tobytes() == starts[3].tobytes()
    assert np.array_equal(b["pose"][1], starts[1], equal_nan=True)
    assert list(b["final"][1]) == [0.0, 0.0] and list(b["final"][3]) == [0.0, 0.0]
    for k in (0, 2, 4):
        for name in ("pose", "status", "trace", "normal", "final"):
            assert b[name][k].tobytes() == clean[name][k].tobytes(), (k, name)
    assert b["best"][0] in (0, 2, 4)
    if clean["best"][0] in (0, 2, 4):
        assert b["best"][0] == clean["best"][0] and b["T_best"].tobytes() == clean["T_best"].tobytes()
    loc.ctx.check_errors(stream())


def test_duplicates_tie_to_the_lower_index(loc, scene, scan, batch18, grid_scores):
    s, w = scene["starts"], batch18.best
    assert w >= 0
    other = [k for k in (0, 3) if k != w]
    got = loc.submit_batch(scan, len(scan), np.stack([s[other[0]], s[w], s[w], s[other[-1]]]), with_normal=True, d2d=True).result()
    same_bits(got.results[1], got.results[2])
    same_bits(got.results[1], batch18.results[w])
    assert got.scores[1] == got.scores[2] == batch18.scores[w] and got.best == 1
    # the scorer and the top-K: a pose given twice keeps the lower index first
    g = scene["grid"]
    top = int(np.argmax(grid_scores[0]))
    poses = np.stack([g[0], g[top], g[1], g[top], g[2]])
    rel = loc.relocalise(scan, len(scan), poses, keep=3, iterations=0, d2d=True).result()
    assert rel.scores[1] == rel.scores[3] == grid_scores[0][top] and list(rel.candidates[:2]) == [1, 3]
    assert rel.batch.best == 0 and rel.index == 1


def test_an_empty_map(scene, scan):
    from sps_amd.localiser import NDTLocaliser
    empty = NDTLocaliser(np.zeros((0, 3)), resolution=RES, leaf=LEAF, source="cells")
    got = empty.submit_batch(scan, len(scan), scene["starts"][:4], d2d=True).result()
    assert got.best == -1 and got.pose.tobytes() == scene["starts"][0].tobytes()
    n_pts, n_src = len(scene["pts"]), scene["src"]["n_src"][1]
    assert [(r.status, r.iterations, r.n_corr, r.n_points, r.n_sources) for r in got.results] == [(2, 1, 0, n_pts, n_src)] * 4
    assert (got.scores == 0.0).all() and (got.counts == 0).all()
    sc, cnt = empty.score_poses(scan, len(scan), scene["grid"], d2d=True).result()
    assert (sc == 0.0).all() and (cnt == 0).all()
    rel = empty.relocalise(scan, len(scan), scene["grid"], keep=3, d2d=True).result()
    assert not rel.ok and list(rel.candidates) == [-1] * 3 and rel.pose.tobytes() == scene["grid"][0].tobytes()
    none = empty.submit_batch(scan, 0, scene["starts"][:2], d2d=True).result()   # and no rows at all
    assert none.best == -1 and [(r.status, r.n_points, r.n_sources) for r in none.results] == [(2, 0, 0)] * 2
    empty.ctx.check_errors(stream())


def test_an_online_map_after_one_integrate(scene, scan):
    from sps_amd.localiser import NDTLocaliser
    dyn = NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF, source="cells", cell_capacity=8192)
    scan2 = sensor_scan(2)
    assert dyn.integrate(dev(scan2), len(scan2), T_TRUE).result().points > 1000
    starts = scene["starts"][[CENTRE, 0, 11]]
    got = dyn.submit_batch(scan, len(scan), starts, with_normal=True, d2d=True).result()
    for k in range(3):
        same_bits(got.results[k], dyn.submit(scan, len(scan), starts[k], with_normal=True).result())
    sc, cnt = dyn.score_poses(scan, len(scan), scene["grid"][:TILE + 1], d2d=True).result()
    zero = dyn.submit_batch(scan, len(scan), scene["grid"][:TILE + 1], iterations=0, d2d=True).result()
    assert zero.scores.tobytes() == sc.tobytes() and zero.counts.tobytes() == cnt.tobytes() and cnt.min() > 0
    dyn.ctx.check_errors(stream())


def test_a_grid_longer_than_one_chunk(loc, scene, grid_scores):
    """the smallest source capacity at which 2 * TILE + 1 poses no longer fit one chunk of the scratch: the second chunk
    overwrites the partial rows of the first, and every pose scores what it scores with a capacity cut to the records"""
    from sps_amd import _native
    P = 2 * TILE + 1
    scratch = _native.lib.sps_ndt_score_d2d_scratch
    blocks = next(b for b in range(1, 1 << 18) if scratch((b - 1) * 32 + 1, P) // (b * 16) < P)
    cap = (blocks - 1) * 32 + 1
    assert scratch(cap, P) // (blocks * 16) == 2 * TILE and scratch(cap - 1, P) // ((blocks - 1) * 16) >= P and cap <= 1 << 23
    rec = DR.records(scene["src"])
    poses = np.concatenate([scene["grid"], scene["starts"], scene["grid"][:2]])[:P]
    assert len(poses) == P
    sc, cnt = raw_score(loc, rec, poses, cap=cap)
    tight = raw_score(loc, rec, poses)
    assert sc.tobytes() == tight[0].tobytes() and cnt.tobytes() == tight[1].tobytes()
    assert sc[:45].tobytes() == grid_scores[0].tobytes() and sc[63:].tobytes() == grid_scores[0][:2].tobytes()


def test_arguments_of_the_two_calls_are_checked(loc, scene):
    from sps_amd import _native
    rec = DR.records(scene["src"])
    r, n = upload(rec, len(rec), len(rec))
    cap = len(rec)
    T = dev(np.tile(np.eye(4), (65, 1, 1)))
    out = torch.zeros(65 * 64, dtype=torch.float64, device="cuda")
    sb = torch.zeros(_native.lib.sps_ndt_align_d2d_batch_scratch(cap, 64), dtype=torch.uint8, device="cuda")
    ss = torch.zeros(_native.lib.sps_ndt_score_d2d_scratch(cap, 64), dtype=torch.uint8, device="cuda")
    p = out.data_ptr()
    ptrs = dict(src=r.data_ptr(), n=n.data_ptr(), T=T.data_ptr(), T_out=p, status=p + 65 * 16 * 8, trace=p + 65 * 18 * 8,
                final=p + 65 * 26 * 8, best=p + 65 * 28 * 8, T_best=p + 65 * 29 * 8, scratch=sb.data_ptr())

    def batch(n_hyp=4, iters=2, neighbours=7, outlier_ratio=0.55, **null):
        q = dict(ptrs, **{k: None for k in null})
        loc.ctx.ndt_align_d2d_batch(q["src"], q["n"], cap, q["T"], n_hyp, iters, neighbours, 50, outlier_ratio, 1e-4, 1e-5, q["T_out"],
                                    q["status"], q["trace"], None, q["final"], q["best"], q["T_best"], q["scratch"], stream())

    def score(n_pose=4, neighbours=7, outlier_ratio=0.55, **null):
        q = dict(ptrs, scratch=ss.data_ptr())
        q.update({k: None for k in null})
        loc.ctx.ndt_score_poses_d2d(q["src"], q["n"], cap, q["T"], n_pose, neighbours, outlier_ratio, q["T_out"], q["scratch"], stream())

    bad_batch = [dict(n_hyp=0), dict(n_hyp=65), dict(neighbours=3), dict(outlier_ratio=1.5), dict(iters=10001), dict(iters=-1)]
    bad_batch += [{k: True} for k in ("src", "n", "T", "T_out", "status", "trace", "final", "best", "T_best", "scratch")]
    for kw in bad_batch:
        with pytest.raises(_native.SpsError) as e:
            batch(**kw)
        assert e.value.code == _native.ERR_INVALID, kw
    bad_score = [dict(n_pose=0), dict(n_pose=65537), dict(neighbours=3), dict(outlier_ratio=0.0)]
    bad_score += [{k: True} for k in ("src", "n", "T", "T_out", "scratch")]
    for kw in bad_score:
        with pytest.raises(_native.SpsError) as e:
            score(**kw)
        assert e.value.code == _native.ERR_INVALID, kw
    batch(n_hyp=64)                                                             # the largest batch is accepted
    score(n_pose=64)
    batch(iters=0, trace=True)                                                  # no iterations need no trace rows
    torch.cuda.synchronize()
    assert _native.lib.sps_ndt_align_d2d_batch_scratch(cap, 65) == -1 and _native.lib.sps_ndt_score_d2d_scratch(cap, 0) == -1
    loc.ctx.check_errors(stream())


# ---- 3. device against restatement ----------------------------------------------------------------------------------------------
def test_batch_matches_the_restatement(batch18, scene, tol):
    """Final scores: the device adds the m per-pair scores of a pose in its fixed order, the restatement with math.fsum; the
    bound (m + 6) * 2^-52 * sum |term| is that of test_hip_ndt_d2d.py::check_one_iteration."""
    ref = scene["ref"]
    worst = 0.0
    for k, (a, b) in enumerate(zip(batch18.results, ref["results"])):
        assert b["faces"] == 0 and b["boundary"] == 0 and ref["hits"][k]["faces"] == 0 and ref["hits"][k]["boundary"] == 0, k
        terms = ref["hits"][k]["terms"][:, 27]
        bound = (len(terms) + 6) * 2.0 ** -52 * math.fsum(np.abs(terms))
        dt, dr = LR.pose_difference(a.pose, b["pose"])
        diff = abs(batch18.scores[k] - ref["scores"][k])
        worst = max(worst, diff / bound, dt / tol[0], dr / tol[1])
        print(f"hypothesis {k:2d}: status {a.status}/{b['status']} iterations {a.iterations}/{b['iterations']} sources "
              f"{a.n_corr}/{b['n_corr']} final {batch18.counts[k]}/{ref['counts'][k]} pose {dt:.3e} m {dr:.3e} rad score "
              f"|diff| {diff:.3e} bound {bound:.3e}")
        assert (a.status, a.iterations, a.n_corr, a.n_sources) == (b["status"], b["iterations"], b["n_corr"], scene["src"]["n_src"][1]), k
        np.testing.assert_array_equal(a.trace[:, 0], b["trace"][:, 0])         # the sources counted in every iteration
        assert batch18.counts[k] == ref["counts"][k], k
        assert dt <= tol[0] and dr <= tol[1], k
        assert diff <= bound, k
    print(f"worst ratio to its bound: {worst:.3f}")
    assert batch18.best == ref["best"]
    assert batch18.pose.tobytes() == batch18.results[batch18.best].pose.tobytes()


def test_grid_scores_match_the_restatement(grid_scores, scene):
    ref = scene["ref_grid"]
    sc, cnt = grid_scores
    assert (ref["faces"] == 0).all() and (ref["boundary"] == 0).all()
    np.testing.assert_array_equal(cnt, ref["counts"])
    bound = (ref["m"] + 6) * 2.0 ** -52 * ref["sum_abs"]
    ratio = np.abs(sc - ref["scores"]) / bound
    print(f"{len(sc)} poses, {ref['m'].min()} to {ref['m'].max()} pairs: worst |device - fsum| / bound {ratio.max():.3f}; against the "
          f"restatement in the device's order {np.abs(sc - ref['ordered']).max():.3e}")
    assert (ratio <= 1.0).all()
    assert int(np.argmax(sc)) == int(np.argmax(ref["scores"]))


# ---- 4. gates and the loop --------------------------------------------------------------------------------------------------------
def test_nobody_qualifying_leaves_the_map_the_carve_and_the_estimator_alone(scene, scan):
    from sps_amd.localiser import NDTLocaliser
    from sps_amd.pose_estimator import PoseEstimator
    dyn = NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF, source="cells", cell_capacity=8192,
                       match_status=dict(max_distance=0.5))
    est = PoseEstimator(T_INIT, "cuda")
    est.predict(0.1)
    opts = dict(min_pass=1, miss_frames=1, through_sigma=2.0)
    before = [a.tobytes() for a in dyn.map_cells()], [a.tobytes() for a in dyn.carve_state()], est.state_dev.cpu().numpy().tobytes()
    far = scene["starts"][:4].copy()
    far[:, 0, 3] += 500.0
    pend = dyn.submit_batch(scan, len(scan), far, integrate=True, carve=True, carve_options=opts, d2d=True)
    est.correct_from(pend)
    res = pend.result()
    assert res.best == -1 and [r.status for r in res.results] == [2] * 4 and res.pose.tobytes() == far[0].tobytes()
    assert (res.map_update.founded, res.map_update.points) == (0, 0) and (res.map_carve.rays, res.map_carve.cleared) == (0, 0)
    assert res.match is not None and res.match.verdict == -1 and not res.match.lost
    after = [a.tobytes() for a in dyn.map_cells()], [a.tobytes() for a in dyn.carve_state()], est.state_dev.cpu().numpy().tobytes()
    assert before == after
    assert est.state().n_correct == 0
    # and where a hypothesis is selected all three run, at its pose
    pend = dyn.submit_batch(scan, len(scan), scene["starts"][[0, CENTRE]], integrate=True, carve=True, carve_options=opts, d2d=True)
    est.correct_from(pend)
    res = pend.result()
    assert res.best >= 0 and res.map_update.points > 1000 and res.map_carve.rays > 1000 and res.match.n_inliers > 0
    assert est.state().n_correct == 1 and [a.tobytes() for a in dyn.map_cells()] != before[0]
    points = NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF, cell_capacity=8192)   # the point path fed that pose
    points.carve(scan, len(scan), res.pose, **opts).result()
    points.integrate(scan, len(scan), res.pose).result()
    for a, b in zip(dyn.map_cells(), points.map_cells()):
        assert a.tobytes() == b.tobytes()
    dyn.ctx.check_errors(stream())


class RestatementOnDevice(DBR.D2DBatchLocaliser):
    """the restatement's single alignment behind a real PendingPose, whose device buffer the estimator's correction reads"""

    def submit(self, rows, count, T_init):
        from sps_amd.localiser import PendingPose, _pose_layout
        r = super().submit(rows, count, T_init).result()
        K = len(r.trace)
        o = _pose_layout(K, False)
        h = np.zeros(o["total"])
        h[o["T_out"]:o["status"]] = r.pose.ravel()
        h[o["status"]:o["n_points"]].view(np.int32)[:] = [r.status, r.iterations, r.n_corr, 0]
        h[o["n_points"]:o["trace"]].view(np.int32)[:] = [r.n_points, r.n_sources]
        h[o["trace"]:o["normal"]] = r.trace.ravel()
        out = dev(h)
        host = torch.from_numpy(h.copy())
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return PendingPose(K, False, host, ev, (None, None, out, None, None))


@pytest.fixture(scope="module")
def sequence():
    """three frames of the loop test of test_hip_ndt_d2d.py: 0.5 m per scan along x, a slow turn"""
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
    return mp, truth, scans, net, step


@pytest.mark.parametrize("mode", ["hypotheses", "search", "estimator"])
def test_three_loop_frames_follow_the_restatement(sequence, tol, mode):
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser, pose_grid
    from sps_amd.pose_estimator import PoseEstimator
    from sps_amd.sps_filters import SPSCVMFilter
    mp, truth, scans, net, step = sequence
    mpt = torch.from_numpy(np.ascontiguousarray(mp[:, :3], dtype=np.float32))
    map64 = mp[:, :3].astype(np.float64)
    ndt = NDTLocaliser(map64, resolution=RES, leaf=LEAF, source="cells")
    kw = dict(hypotheses=dict(hypotheses=pose_grid((0.0, step), 0.0, 0.0)),
              search=dict(search=pose_grid((0.0, step, -step), (0.0, 0.5), (0.0, 4.0)), search_keep=3), estimator={})[mode]

    def run(localiser):
        est = PoseEstimator(truth[0], "cuda", initial_velocity=(step / 0.1, 0.0, 0.0)) if mode == "estimator" else None
        loop = LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0), localiser, truth[0],
                                estimator=est, d2d=True, **kw)
        steps = [loop.step(s, **(dict(dt=0.1) if est is not None else {})) for s in scans]
        return loop, steps

    loop, steps = run(ndt)
    ref_loop, ref_steps = run(RestatementOnDevice(NR.cells(map64, RES), ndt))
    assert loop.device_guess is (mode == "estimator") and ref_loop.device_guess is False
    for i, (s, t) in enumerate(zip(steps, ref_steps)):
        a, b = s.pose_result, t.pose_result
        dt, dr = LR.pose_difference(loop.poses[i], ref_loop.poses[i])
        print(f"{mode} frame {i}: status {a.status}/{b.status} iterations {a.iterations}/{b.iterations} sources {a.n_corr}/{b.n_corr} "
              f"of {a.n_sources}/{b.n_sources} flagged {s.flagged}/{t.flagged}; device vs restatement {dt:.3e} m {dr:.3e} rad")
        assert (a.status, a.iterations, a.n_corr, a.n_points, a.n_sources) == (b.status, b.iterations, b.n_corr, b.n_points, b.n_sources), i
        assert s.flagged == t.flagged and not s.flagged, i
        assert dt <= tol[0] and dr <= tol[1], i
        if mode == "estimator":
            assert s.batch is not None and len(s.batch.results) == 1 and s.estimate is not None, i
            et, er = LR.pose_difference(s.estimate, t.estimate)
            assert et <= tol[0] and er <= tol[1], i
        else:
            # hypotheses: every frame is a batch; search: frame 0 is the search and its batch, the frames after it plain ones
            assert (s.search is not None) == (t.search is not None) == (mode == "search" and i == 0), i
            assert (s.batch is not None) == (t.batch is not None) == (mode == "hypotheses" or i == 0), i
            if s.batch is not None:
                assert s.batch.best == t.batch.best and [r.status for r in s.batch.results] == [r.status for r in t.batch.results], i
                assert list(s.batch.counts) == list(t.batch.counts), i
            if s.search is not None:
                assert list(s.search.candidates) == list(t.search.candidates) and s.search.index == t.search.index, i
    ndt.ctx.check_errors(stream())


# ---- 5. unchanged behaviour, bit for bit -------------------------------------------------------------------------------------------
def test_without_the_keyword_nothing_changes(loc, scene, scan, batch18):
    from sps_amd.localiser import NDTLocaliser
    from tests.test_hip_ndt_d2d import raw_align
    fresh = NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF, source="cells")   # never saw a d2d=True call
    a = loc.submit(scan, len(scan), T_INIT, with_normal=True).result()
    b = fresh.submit(scan, len(scan), T_INIT, with_normal=True).result()
    same_bits(a, b)
    raw = raw_align(fresh, DR.records(scene["src"]))
    assert a.pose.tobytes() == raw["pose"].tobytes() and a.normal.tobytes() == raw["normal"].tobytes() and a.iterations > 1
    T_dev = dev(np.eye(4).reshape(16))
    poses = np.eye(4)[None]
    for L in (loc, fresh):
        for call in (lambda **kw: L.submit_batch(scan, len(scan), poses, **kw), lambda **kw: L.score_poses(scan, len(scan), poses, **kw),
                     lambda **kw: L.relocalise(scan, len(scan), poses, **kw),
                     lambda **kw: L.submit_from_device(scan, len(scan), T_dev, **kw)):
            for kw in ({}, dict(d2d=False)):
                with pytest.raises(ValueError, match=OLD_TEXT):
                    call(**kw)
    one = NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF)
    two = NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF)
    pa = one.submit_batch(scan, len(scan), scene["starts"][:5], with_normal=True, d2d=False).result()
    pb = two.submit_batch(scan, len(scan), scene["starts"][:5], with_normal=True).result()
    same_batch(pa, pb)
    assert all(r.n_sources == 0 for r in pa.results) and pa.results[0].iterations > 1
    sa, sb = one.score_poses(scan, len(scan), scene["grid"], d2d=False).result(), two.score_poses(scan, len(scan), scene["grid"]).result()
    assert sa[0].tobytes() == sb[0].tobytes() and sa[1].tobytes() == sb[1].tobytes() and sa[1].min() > 0
    for call in (lambda: one.submit_batch(scan, len(scan), poses, d2d=True), lambda: one.score_poses(scan, len(scan), poses, d2d=True),
                 lambda: one.relocalise(scan, len(scan), poses, d2d=True),
                 lambda: one.submit_from_device(scan, len(scan), T_dev, d2d=True)):
        with pytest.raises(ValueError, match="d2d=True needs an NDTLocaliser with source='cells'"):
            call()
    with pytest.raises(ValueError, match="d2d=True and coarse_to_fine exclude each other"):
        loc.submit_batch(scan, len(scan), poses, d2d=True, coarse_to_fine=True)
    loc.ctx.check_errors(stream())
