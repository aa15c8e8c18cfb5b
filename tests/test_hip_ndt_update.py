"""GPU tests of the online NDT map (sps_amd.localiser.NDTLocaliser(..., cell_capacity=N); C ABI: the "NDT localiser, online
map" section of include/sps_hip.h) against the numpy restatement in tests/ndt_update_reference.py.  Shapes are those of
test_hip_ndt.py: the 57 k-point synthetic map, 12.8 k-point scans thinned at leaf 0.4 to ~4.2 k points.  There is no exp
and no open sum order on the update's path, so the map is compared bit for bit."""
import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_reference as NR
from tests import ndt_update_reference as UR
from tests.helpers import CFG, net_from_params
from tests.test_ndt_cpu import KW, LEAF, T_INIT, T_TRUE, sensor_scan
from tests.test_ndt_update_cpu import changed_scene, hand_points

pytestmark = pytest.mark.gpu

RES = 1.0
TOL_FLOOR = 1e-12
CAPACITY = 4096
FIELDS = ("keys", "count", "mean", "icov", "valid")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def make(map_xyz, capacity=CAPACITY, **kw):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(map_xyz, resolution=RES, leaf=LEAF, cell_capacity=capacity, **kw)


def cells_of(loc):
    return dict(zip(FIELDS, loc.map_cells()))


def raw_cells(loc, C=None):
    """sps_ndt_map_cells itself: every row the context holds (the capacity, for an online map)"""
    C = loc.cell_capacity if C is None else C
    key = torch.zeros(C, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(C, dtype=torch.int32, device="cuda")
    mean = torch.zeros((C, 3), dtype=torch.float64, device="cuda")
    icov = torch.zeros((C, 6), dtype=torch.float64, device="cuda")
    valid = torch.zeros(C, dtype=torch.int32, device="cuda")
    loc.ctx.ndt_map_cells(key.data_ptr(), cnt.data_ptr(), mean.data_ptr(), icov.data_ptr(), valid.data_ptr())
    return dict(keys=key.cpu().numpy().view(np.uint64), count=cnt.cpu().numpy(), mean=mean.cpu().numpy(), icov=icov.cpu().numpy(),
                valid=valid.cpu().numpy().astype(bool))


def assert_same_cells(got, want, what=""):
    for k in FIELDS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if k in ("mean", "icov"):
            assert a.tobytes() == b.tobytes(), (what, k, int((a != b).sum()))
        else:
            np.testing.assert_array_equal(a.astype(np.int64) if k != "keys" else a, b.astype(np.int64) if k != "keys" else b, str((what, k)))


def assert_map_is(loc, m, what=""):
    """the device map against the restatement's: the assigned cells in id order, the rest of the capacity empty"""
    assert_same_cells(cells_of(loc), m, what)
    assert_same_cells(raw_cells(loc), UR.rows_by_capacity(m), what)
    assert loc.map_info() == (len(m["keys"]), m["capacity"], m["dropped"])


def raw_update(loc, pts, n, cap, T, gate=None, max_cell_points=0, T_on_device=False):
    """sps_ndt_map_update itself on float64 points: returns info as a list"""
    from sps_amd import _native
    buf = np.zeros((max(cap, len(pts), 1), 3))
    buf[:len(pts)] = pts
    p = dev(buf)
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    scratch = torch.empty(_native.lib.sps_ndt_map_update_scratch(cap), dtype=torch.uint8, device="cuda")
    g = None if gate is None else torch.tensor([gate], dtype=torch.int32, device="cuda")
    Td = dev(np.asarray(T, dtype=np.float64).reshape(16)) if T_on_device else None
    loc.ctx.ndt_map_update(p.data_ptr(), n_dev.data_ptr(), cap, None if T_on_device else T, Td.data_ptr() if T_on_device else None,
                           g.data_ptr() if g is not None else None, max_cell_points, info.data_ptr(), scratch.data_ptr(), stream())
    out = [int(v) for v in info.cpu().numpy()]
    loc.ctx.check_errors(stream())
    return out


def same_bits(a, b):
    assert (a.status, a.iterations, a.n_corr, a.n_points) == (b.status, b.iterations, b.n_corr, b.n_points)
    for x, y in ((a.pose, b.pose), (a.trace, b.trace), (a.normal, b.normal)):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()


@pytest.fixture(scope="module")
def map_xyz():
    hb, _ = NR.hand_built_cells()
    return np.concatenate([synthetic.build_map(**KW)[:, :3].astype(np.float64), hb])


@pytest.fixture(scope="module")
def scans():
    """sensor scans 1 .. 4 taken at T_TRUE and their thinned float64 points (read-only)"""
    out = {}
    for seed in (1, 2, 3, 4):
        s = sensor_scan(seed)
        out[seed] = (s, LR.downsample(s, len(s), LEAF)[1])
    return out


@pytest.fixture(scope="module")
def static(map_xyz):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(map_xyz, resolution=RES, leaf=LEAF)


# ---- static equivalence ------------------------------------------------------------------------------------------------
def test_a_dynamic_map_before_any_update_is_the_static_map(static, map_xyz, scans):
    from sps_amd.localiser import pose_grid
    dyn = make(map_xyz)
    want = cells_of(static)
    assert_same_cells(cells_of(dyn), want)
    raw = raw_cells(dyn)
    n = len(want["keys"])
    assert len(raw["keys"]) == CAPACITY and (raw["keys"][n:] == UR.EMPTY_KEY).all() and not raw["count"][n:].any()
    assert not raw["valid"][n:].any() and not raw["mean"][n:].any() and not raw["icov"][n:].any()
    assert dyn.map_info() == (n, CAPACITY, 0)
    scan = dev(scans[1][0])
    a, b = static(scan, len(scan), T_INIT, with_normal=True), dyn(scan, len(scan), T_INIT, with_normal=True)
    assert a.status == 0 and a.map_update is None and b.map_update is None
    same_bits(a, b)
    starts = T_INIT @ pose_grid([0.0], [0.0, 2.0], [0.0, 15.0])[:3]
    ba, bb = static.submit_batch(scan, len(scan), starts).result(), dyn.submit_batch(scan, len(scan), starts).result()
    assert ba.best == bb.best >= 0 and ba.scores.tobytes() == bb.scores.tobytes() and (ba.counts == bb.counts).all()
    for x, y in zip(ba.results, bb.results):
        same_bits(x, y)
    assert ba.pose.tobytes() == bb.pose.tobytes() and bb.map_update is None
    poses = T_INIT @ pose_grid([0.0, 1.0], [0.0], [-10.0, 0.0, 10.0])[:5]
    sa, ca = static.score_poses(scan, len(scan), poses).result()
    sb, cb = dyn.score_poses(scan, len(scan), poses).result()
    assert sa.tobytes() == sb.tobytes() and (ca == cb).all() and ca.max() > 1000
    dyn.ctx.check_errors(stream())


# ---- one update ----------------------------------------------------------------------------------------------------------
def test_one_update_matches_the_restatement(map_xyz, scans):
    scan, pts = scans[1]
    shifted = LR.perturbation(0.0, 9.0, 0.0, 0.0) @ T_TRUE                     # 9 m to the side: existing and new cells
    dyn = make(map_xyz)
    m = UR.build(map_xyz, CAPACITY)
    n0 = len(m["keys"])
    want = UR.update(m, pts, shifted)
    got = dyn.integrate(dev(scan), len(scan), shifted).result()
    print("info (cells, founded, dropped, points):", want)
    assert (got.cells, got.founded, got.dropped, got.points, got.n_points) == (*want, len(pts))
    assert want[1] > 100 and want[3] == len(pts) and want[0] - n0 == want[1]  # founded cells follow in founder order
    assert (m["count"][:n0] != UR.build(map_xyz, CAPACITY)["count"]).sum() > 100   # and existing cells were merged into
    assert_map_is(dyn, m)
    dyn.ctx.check_errors(stream())


def test_one_context_rebuilt_dynamic_static_dynamic():
    """Both builds own the context's map through one routine: each replaces what the other left."""
    from sps_amd import _native
    from sps_amd.datasets.blt_dataset import radius_grid_cells
    rng = np.random.default_rng(11)
    mp = 0.05 + 1.9 * rng.random((300, 3))                                     # the 8 cells of [0, 2)^3
    pts = 0.05 + np.array([2.9, 1.9, 1.9]) * rng.random((50, 3))               # those and the 4 cells at 2 <= x < 3
    dyn = make(mp, capacity=16)                                                # the first dynamic build
    xyz = dev(mp)
    keys, start, idx = radius_grid_cells(xyz, RES)
    keys = keys.contiguous()
    args = (keys.data_ptr(), start.data_ptr(), idx.data_ptr(), xyz.data_ptr(), len(keys), len(mp), RES, 6, 0.01)
    assert len(keys) == 8 and dyn.map_info() == (8, 16, 0)
    dyn.ctx.ndt_map_build(*args, stream())
    with pytest.raises(_native.SpsError):
        raw_update(dyn, pts, len(pts), len(pts), np.eye(4))
    with pytest.raises(_native.SpsError):
        dyn.ctx.ndt_map_info()
    assert_same_cells(raw_cells(dyn, 8), NR.cells(mp, RES))                    # the static map holds its 8 rows
    dyn.ctx.ndt_map_build_dynamic(*args, 16, stream())
    m = UR.build(mp, 16)
    assert_map_is(dyn, m)
    want = UR.update(m, pts, np.eye(4))
    assert raw_update(dyn, pts, len(pts), len(pts), np.eye(4)) == want and want[1] == 4 and want[3] == 50
    assert_map_is(dyn, m)
    dyn.ctx.check_errors(stream())


def test_an_empty_map_plus_one_update_equals_the_static_build(scans):
    from sps_amd.localiser import NDTLocaliser
    scan, pts = scans[2]
    dyn = make(np.zeros((0, 3)))
    assert dyn.map_info() == (0, CAPACITY, 0) and len(dyn.map_cells()[0]) == 0
    res = dyn.integrate(dev(scan), len(scan), T_TRUE).result()
    q = LR.transform(pts, T_TRUE)
    want = cells_of(NDTLocaliser(q, resolution=RES, leaf=LEAF))
    got = cells_of(dyn)
    assert res.founded == res.cells == len(want["keys"]) > 500 and res.points == len(pts)
    o = np.argsort(got["keys"], kind="stable")
    assert_same_cells({k: got[k][o] for k in FIELDS}, want)
    assert want["valid"].sum() > 50
    # and a localiser can start from it
    a = dyn(dev(scan), len(scan), T_INIT)
    assert a.status in (0, 1) and a.n_corr > 1000


# ---- edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_edge_counts(scans, n):
    pts = scans[3][1]
    dyn = make(np.zeros((0, 3)), capacity=512)
    m = UR.build(np.zeros((0, 3)), 512)
    assert raw_update(dyn, pts[:300], n, 300, T_TRUE) == UR.update(m, pts[:300], T_TRUE, n=n)
    assert_map_is(dyn, m, n)
    # once more on the cells that now exist, with the pose on the device
    assert raw_update(dyn, pts[:300], n, 300, T_TRUE, T_on_device=True) == UR.update(m, pts[:300], T_TRUE, n=n)
    assert_map_is(dyn, m, n)


def test_cap_below_the_count_bad_points_and_small_cells():
    hb, names = NR.hand_built_cells()
    pts = hand_points()
    dyn = make(hb, capacity=16)
    m = UR.build(hb, 16)
    five = int(np.nonzero(m["keys"] == NR.cell_key(names["five"]))[0][0])
    assert m["count"][five] == 5 and not m["valid"][five]
    # cap = 4 < *n_dev = 8: points 0 .. 3, of which index 2 is NaN
    assert raw_update(dyn, pts, 8, 4, np.eye(4)) == UR.update(m, pts, np.eye(4), cap=4, n=8) == [8, 3, 0, 3]
    assert_map_is(dyn, m)
    # all eight: the NaN and the point beyond the guard are skipped and not counted; C and D are single-point cells
    assert raw_update(dyn, pts, 8, 8, np.eye(4)) == UR.update(m, pts, np.eye(4)) == [9, 1, 0, 6]
    assert_map_is(dyn, m)
    got = cells_of(dyn)
    assert list(got["count"][5:]) == [3, 3, 2, 1] and not got["valid"][8] and not got["valid"][5:8].any()   # min_points = 6
    # the five-point cell gets its sixth point
    p = np.asarray(names["five"], dtype=np.float64)[None] + [[0.5, 0.4, 0.6]]
    assert raw_update(dyn, p, 1, 1, np.eye(4)) == UR.update(m, p, np.eye(4)) == [9, 0, 0, 1]
    assert_map_is(dyn, m)
    got = cells_of(dyn)
    assert got["count"][five] == 6 and got["valid"][five]


def test_the_capacity_rule():
    hb, _ = NR.hand_built_cells()
    pts = hand_points()                                                        # four new cells, founders 0, 1, 3, 6
    dyn = make(hb, capacity=7)
    m = UR.build(hb, 7)
    assert len(m["keys"]) == 5
    assert raw_update(dyn, pts, 8, 8, np.eye(4)) == UR.update(m, pts, np.eye(4)) == [7, 2, 2, 4]
    assert_map_is(dyn, m)
    assert [int(k) for k in cells_of(dyn)["keys"][5:]] == [int(NR.cell_key(np.array(c))) for c in ([0, 0, 0], [5, 0, 0])]
    assert raw_update(dyn, pts, 8, 8, np.eye(4)) == UR.update(m, pts, np.eye(4)) == [7, 0, 2, 4]
    assert_map_is(dyn, m)
    assert dyn.map_info() == (7, 7, 4)
    scan = sensor_scan(1)
    assert dyn(dev(scan), len(scan), T_INIT).status == 2                       # the full table still answers lookups


def test_forgetting_bites_on_one_cell_and_not_on_its_neighbour():
    rng = np.random.default_rng(3)
    big = 0.1 + 0.8 * rng.random((40, 3))
    small = np.array([1.0, 0.0, 0.0]) + 0.1 + 0.8 * rng.random((8, 3))
    mp = np.concatenate([big, small])
    dyn = make(mp, capacity=4)
    m = UR.build(mp, 4)
    assert list(m["count"]) == [40, 8]
    S_small = m["S"][1].copy()
    p = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]])
    assert raw_update(dyn, p, 2, 2, np.eye(4), max_cell_points=10) == UR.update(m, p, np.eye(4), max_cell_points=10)
    assert list(m["count"]) == [11, 9]
    assert_map_is(dyn, m)
    plain = UR.build(mp, 4)
    UR.update(plain, p, np.eye(4))
    assert plain["S"][1].tobytes() == m["S"][1].tobytes() != S_small.tobytes()       # the neighbour merged as without a cap
    assert plain["icov"][0].tobytes() != m["icov"][0].tobytes()                      # the capped cell did not


# ---- the gate ------------------------------------------------------------------------------------------------------------
def test_the_gate_follows_the_status_on_the_device(map_xyz, scans):
    scan, pts = scans[1]
    closed = make(map_xyz, min_correspondences=len(pts) + 1)
    before = raw_cells(closed)
    r = closed.submit(dev(scan), len(scan), T_INIT, integrate=True).result()
    n0 = len(cells_of(closed)["keys"])
    assert r.status == 2 and (r.map_update.cells, r.map_update.founded, r.map_update.dropped, r.map_update.points) == (n0, 0, 0, 0)
    assert_same_cells(raw_cells(closed), before)
    assert closed.map_info() == (n0, CAPACITY, 0)
    # the same through best[1] of a batch in which nobody qualifies
    b = closed.submit_batch(dev(scan), len(scan), np.stack([T_INIT, T_TRUE]), integrate=True).result()
    assert b.best == -1 and (b.map_update.cells, b.map_update.founded, b.map_update.points) == (n0, 0, 0)
    assert_same_cells(raw_cells(closed), before)
    assert raw_update(closed, pts, len(pts), len(pts), T_TRUE, gate=3) == [n0, 0, 0, 0]
    assert_same_cells(raw_cells(closed), before)
    # status 0 opens it: the map becomes the restatement's update at the pose the device found
    opened = make(map_xyz)
    m = UR.build(map_xyz, CAPACITY)
    r = opened.submit(dev(scan), len(scan), T_INIT, integrate=True).result()
    assert r.status == 0
    want = UR.update(m, pts, r.pose, gate=r.status)
    u = r.map_update
    assert [u.cells, u.founded, u.dropped, u.points] == want and want[3] == len(pts)
    assert_map_is(opened, m)
    # a batch with a selected hypothesis integrates at its pose
    opened = make(map_xyz)
    m = UR.build(map_xyz, CAPACITY)
    b = opened.submit_batch(dev(scan), len(scan), np.stack([T_INIT, T_TRUE]), integrate=True).result()
    assert b.best >= 0
    want = UR.update(m, pts, b.pose)
    assert [b.map_update.cells, b.map_update.founded, b.map_update.dropped, b.map_update.points] == want
    assert_map_is(opened, m)
    opened.ctx.check_errors(stream())


def test_relocalise_integrates_at_the_selected_pose(map_xyz, scans):
    from sps_amd.localiser import pose_grid
    scan, pts = scans[2]
    loc = make(map_xyz)
    m = UR.build(map_xyz, CAPACITY)
    r = loc.relocalise(dev(scan), len(scan), T_INIT @ pose_grid([0.0, 1.0], [0.0], [-10.0, 0.0, 10.0])[:5], keep=2,
                       integrate=True).result()
    assert r.ok and r.batch.best >= 0 and r.map_update is r.batch.map_update
    want = UR.update(m, pts, r.pose)
    u = r.map_update
    assert [u.cells, u.founded, u.dropped, u.points] == want and want[3] == len(pts)
    assert_map_is(loc, m)
    loc.ctx.check_errors(stream())


# ---- determinism ---------------------------------------------------------------------------------------------------------
def test_two_localisers_end_with_the_same_map(map_xyz, scans):
    maps = []
    for _ in range(2):
        dyn = make(map_xyz)
        for seed, dy in ((1, 0.0), (2, 6.0), (3, 6.0)):
            s = dev(scans[seed][0])
            dyn.integrate(s, len(s), LR.perturbation(0.0, dy, 0.0, 0.0) @ T_TRUE, max_cell_points=50)
        maps.append(raw_cells(dyn))
    assert_same_cells(maps[0], maps[1])
    assert maps[0]["count"].max() > 50


# ---- stream order --------------------------------------------------------------------------------------------------------
def test_an_alignment_behind_an_update_on_a_side_stream_sees_the_updated_map(scans):
    sc = changed_scene()
    dyn = make(sc["cut"])
    s1, s2 = dev(scans[1][0]), dev(scans[2][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pa = dyn.submit(s1, len(s1), T_INIT, integrate=True)
        pb = dyn.submit(s2, len(s2), T_INIT)                                   # no synchronisation in between
    a, b = pa.result(), pb.result()
    m = UR.build(sc["cut"], CAPACITY)
    plain = NR.align(scans[2][1], UR.as_cmap(m), T_INIT)
    assert a.status == 0 and UR.update(m, scans[1][1], a.pose)[1] > 100
    fwd = NR.align(scans[2][1], UR.as_cmap(m), T_INIT)
    rev = NR.align(scans[2][1], UR.as_cmap(m), T_INIT, reverse=True)
    spread_t, spread_r = LR.pose_difference(fwd["pose"], rev["pose"])
    tol_t, tol_r = max(100.0 * spread_t, TOL_FLOOR), max(100.0 * spread_r, TOL_FLOOR)
    dt, dr = LR.pose_difference(b.pose, fwd["pose"])
    print(f"spread {spread_t:.3e} m {spread_r:.3e} rad; device vs restatement {dt:.3e} m {dr:.3e} rad; counted {b.n_corr} "
          f"(without the update {plain['n_corr']})")
    assert fwd["faces"] == 0 and fwd["boundary"] == 0
    assert (b.status, b.iterations) == (fwd["status"], fwd["iterations"])
    np.testing.assert_array_equal(b.trace[:, 0], fwd["trace"][:, 0])
    assert dt <= tol_t and dr <= tol_r
    assert b.n_corr > plain["n_corr"]
    assert_map_is(dyn, m)


# ---- the loop ------------------------------------------------------------------------------------------------------------
class RestatementLocaliser:
    """tests/ndt_reference.py and tests/ndt_update_reference.py behind the interface LocalisationLoop uses"""

    def __init__(self, m, like):
        self.m, self.like, self.device, self.cell_capacity = m, like, like.device, m["capacity"]

    def submit_filtered(self, pending, T_init, integrate=False, max_cell_points=0):
        from sps_amd.localiser import PoseResult
        n = int(pending.count_dev.item())
        rows = pending._filtered[:n].cpu().numpy()
        L = self.like
        _, pts = LR.downsample(rows, n, L.leaf, L.capacity)
        r = NR.align(pts, UR.as_cmap(self.m), T_init, L.iterations, L.neighbours, L.min_correspondences, L.outlier_ratio, L.tol_t,
                     L.tol_r)
        if integrate:
            UR.update(self.m, pts, r["pose"], gate=r["status"], max_cell_points=max_cell_points)
        res = PoseResult(r["pose"], r["status"], r["iterations"], r["n_corr"], float("nan"), r["trace"], None, len(pts))

        class Done:
            def result(self):
                return res
        return Done()


def test_the_loop_learns_a_changed_scene(scans):
    from sps_amd.localiser import LocalisationLoop
    from sps_amd.sps_filters import SPSCVMFilter
    sc = changed_scene()
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(np.ascontiguousarray(sc["cut"], dtype=np.float32))
    frames = [scans[k][0] for k in (1, 2, 3, 4)]

    def run(localiser, **kw):
        f = SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0)     # every point passes
        loop = LocalisationLoop(f, localiser, T_INIT, **kw)
        return [loop.step(s) for s in frames]

    fwd = NR.align(scans[1][1], NR.cells(sc["cut"], RES), T_INIT)
    rev = NR.align(scans[1][1], NR.cells(sc["cut"], RES), T_INIT, reverse=True)
    spread_t, spread_r = LR.pose_difference(fwd["pose"], rev["pose"])
    tol_t, tol_r = max(100.0 * spread_t, TOL_FLOOR), max(100.0 * spread_r, TOL_FLOOR)
    like = make(sc["cut"])
    got = run(like, update_map=True)
    want = run(RestatementLocaliser(UR.build(sc["cut"], CAPACITY), like), update_map=True)
    off = run(make(sc["cut"]), update_map=False)
    none = run(make(sc["cut"]))
    for i in range(4):
        a, b = got[i].pose_result, want[i].pose_result
        dt, dr = LR.pose_difference(got[i].pose, want[i].pose)
        print(f"frame {i}: status {a.status}/{b.status} iterations {a.iterations}/{b.iterations} count {a.n_corr}/{b.n_corr} "
              f"(no update: {off[i].pose_result.n_corr}) device vs restatement {dt:.3e} m {dr:.3e} rad; update {a.map_update}")
        assert (a.status, a.iterations, a.n_corr, a.n_points) == (b.status, b.iterations, b.n_corr, b.n_points), i
        assert dt <= tol_t and dr <= tol_r, i
        assert a.map_update is not None and a.map_update.points == a.n_points and not got[i].flagged
        same_bits(off[i].pose_result, none[i].pose_result)
        assert off[i].pose.tobytes() == none[i].pose.tobytes() and off[i].pose_result.map_update is None
    assert got[3].pose_result.n_corr > off[3].pose_result.n_corr
    like.ctx.check_errors(stream())


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_errors(static, map_xyz, scans):
    from sps_amd import _native
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser
    scan = dev(scans[1][0])
    with pytest.raises(ValueError):
        static.integrate(scan, len(scan), T_TRUE)
    with pytest.raises(ValueError):
        static.submit(scan, len(scan), T_INIT, integrate=True)
    with pytest.raises(ValueError):
        static.submit_batch(scan, len(scan), T_INIT[None], integrate=True)
    with pytest.raises(ValueError):
        static.relocalise(scan, len(scan), T_INIT[None], keep=1, integrate=True)
    with pytest.raises(ValueError):
        LocalisationLoop(None, static, T_INIT, update_map=True)
    with pytest.raises(ValueError):
        NDTLocaliser(map_xyz, resolution=RES, leaf=LEAF, cell_capacity=100)    # the map has ~2.5 k cells
    with pytest.raises(ValueError):
        NDTLocaliser(map_xyz[:10], cell_capacity=0)
    with pytest.raises(_native.SpsError):                                      # the C ABI refuses a static map too
        raw_update(static, scans[1][1][:10], 10, 10, T_TRUE)
    assert _native.lib.sps_ndt_map_update_scratch(65537) == -1 and _native.lib.sps_version() == 202
    static.ctx.check_errors(stream())
