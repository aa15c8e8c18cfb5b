"""GPU tests of the scan-matching status (C ABI: the "localiser, scan-matching status" section of include/sps_hip.h;
sps_amd.localiser: ``match_status=`` on both localisers, ``LocalisationLoop(..., recover=...)``) against the
numpy restatement in tests/match_status_reference.py.  The raw calls run on a lattice map whose distances are exact; the
scene is that of tests/test_match_status_cpu.py, whose table says what the threshold 0.85 rests on."""
import math

import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import match_status_reference as MR
from tests import ndt_reference as NR
from tests.helpers import CFG, net_from_params
from tests.test_match_status_cpu import KW, T_INIT, T_TRUE, THRESHOLD, sensor_scan

pytestmark = pytest.mark.gpu

LEAF = 0.4
SENTINEL = -7.5
OPTS = dict(min_inlier_fraction=THRESHOLD)
T_KIDNAPPED = [T_TRUE @ LR.perturbation(10.0, 0.0, 0.0, 0.0), T_TRUE @ LR.perturbation(0.0, 0.0, 0.0, 90.0)]
# sensor -> map of the raw cases: q = (-py, px, pz + 0.25), every entry and every sum exact
T_LATTICE = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.25], [0.0, 0.0, 0.0, 1.0]])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def new_context(xyz, cell):
    """a native context with the radius grid of ``xyz`` (float64 [m, 3]) at cell = r = ``cell``"""
    from sps_amd import _native
    from sps_amd.datasets.blt_dataset import radius_grid_cells
    ctx = _native.Context(0)
    if len(xyz):
        x = dev(xyz)
        keys, start, pts = radius_grid_cells(x, cell)
        ctx.radius_grid_upload(keys.contiguous().data_ptr(), start.data_ptr(), pts.data_ptr(), x.data_ptr(), len(keys), len(xyz),
                               cell, cell, stream())
    else:
        ctx.radius_grid_upload(None, None, None, None, 0, 0, cell, cell, stream())
    return ctx


def raw_status(ctx, pts, n, cap, T, gate=None, max_distance=0.5, max_range=None, min_inlier_fraction=0.0, max_error=math.inf,
               min_valid=1):
    """sps_loc_match_status itself on float64 points -> (the 48 bytes of out_dev, d2_dev as an array of max(cap, 1) rows)"""
    from sps_amd import _native
    buf = np.zeros((max(cap, len(pts), 1), 3))
    buf[:len(pts)] = pts
    p, Td = dev(buf), dev(np.asarray(T, dtype=np.float64).reshape(16))
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    out = torch.full((6,), SENTINEL, dtype=torch.float64, device="cuda")
    d2 = torch.full((max(cap, 1),), SENTINEL, dtype=torch.float64, device="cuda")
    words = None if gate is None else torch.tensor([7, gate], dtype=torch.int32, device="cuda")   # the gate is the second word
    scratch = torch.empty(_native.lib.sps_loc_match_status_scratch(cap), dtype=torch.uint8, device="cuda")
    ctx.loc_match_status(p.data_ptr(), n_dev.data_ptr(), cap, Td.data_ptr(), None if gate is None else words.data_ptr() + 4,
                         max_distance, -1.0 if max_range is None else max_range, min_inlier_fraction, max_error, min_valid,
                         out.data_ptr(), d2.data_ptr(), scratch.data_ptr(), stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), d2.cpu().numpy()


def assert_raw_is(ctx, map_xyz, pts, n, cap, what="", **kw):
    want = MR.status(pts, n, cap, T_LATTICE, map_xyz, 0.5, gate_in=kw.get("gate"), **{k: v for k, v in kw.items() if k != "gate"})
    out, d2 = raw_status(ctx, pts, n, cap, T_LATTICE, **kw)
    assert out == MR.out_bytes(want), (what, np.frombuffer(out[:32]), np.frombuffer(out[32:], dtype=np.int32), want)
    assert d2[:want["n"]].tobytes() == want["d2"].tobytes(), what
    assert (d2[want["n"]:] == SENTINEL).all(), what                       # rows past n are not written
    return want


# ---- the raw ABI on a lattice ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice():
    """12^3 map points at 0.25 m spacing from the origin, in a shuffled order, on a grid of cell 0.5"""
    g = 0.25 * np.arange(12)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    xyz = np.ascontiguousarray(xyz[np.random.default_rng(3).permutation(len(xyz))])
    return new_context(xyz, 0.5), xyz


def sensor_points(q):
    """the sensor-frame points that T_LATTICE moves to q, exactly"""
    q = np.asarray(q, dtype=np.float64)
    return np.stack([q[:, 1], -q[:, 0], q[:, 2] - 0.25], axis=1)


EPS = 2.0 ** -53
SPECIAL_Q = [(-0.5, 0.0, 0.0),                 # 0: exactly max_distance from the corner: an inlier
             (-0.5 - EPS, 0.0, 0.0),           # 1: one ulp further: not one
             (0.125, 0.5, 0.5),                # 2: two map points at the same distance
             (0.125, 0.125, 0.125),            # 3: eight of them
             (10.0, 10.0, 10.0),               # 4: its 27 cells are empty
             (0.5 * 1048576.0, 0.0, 0.0),      # 5: beyond the key range
             (1.0, 1.0, 1.0),                  # 6: on a map point
             (3.25, 1.0, 1.0)]                 # 7: exactly max_distance behind the last plane


@pytest.fixture(scope="module")
def lattice_points():
    """the special points, a NaN and an inf row, then points on a 1/64 raster in and around the lattice: 9 * 32 + 1 rows"""
    rng = np.random.default_rng(4)
    fill = rng.integers(-64, 4 * 64, size=(9 * 32 + 1 - len(SPECIAL_Q) - 2, 3)) / 64.0
    pts = np.concatenate([sensor_points(SPECIAL_Q), [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]], sensor_points(fill)])
    np.testing.assert_array_equal(MR.transform(pts[:len(SPECIAL_Q)], T_LATTICE), np.array(SPECIAL_Q))
    return pts


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 8 * 32 - 1, 8 * 32, 8 * 32 + 1, 9 * 32 + 1])
def test_the_raw_call_equals_the_restatement_bit_for_bit(lattice, lattice_points, n):
    ctx, xyz = lattice
    want = assert_raw_is(ctx, xyz, lattice_points, n, 9 * 32 + 1, n, min_inlier_fraction=0.5, max_error=0.2)
    if n >= 33:                                                            # what the special rows are there for
        d2 = want["d2"]
        assert d2[0] == 0.25 and d2[1] == math.inf and d2[2] == 0.015625 and d2[3] == 3 * 0.015625
        assert d2[4] == math.inf and d2[5] == math.inf and d2[6] == 0.0 and d2[7] == 0.25 and d2[8] == -1.0 and d2[9] == -1.0
        assert 0 < want["n_inliers"] < want["n_valid"] == n - 2
    ctx.check_errors(stream())


def test_the_raw_call_at_its_other_edges(lattice, lattice_points):
    ctx, xyz = lattice
    pts = lattice_points
    assert_raw_is(ctx, xyz, pts, 500, 40, "n_dev > cap")
    w = assert_raw_is(ctx, xyz, pts, -3, 40, "n_dev < 0")
    assert (w["n"], w["verdict"]) == (0, MR.LOST)
    assert_raw_is(ctx, xyz, pts, 0, 0, "cap = 0")
    for gate in (0, 1, 2, 3, -1):                                          # 2, 3 and -1 pass through, whatever the thresholds say
        for frac in (0.0, 0.99):
            w = assert_raw_is(ctx, xyz, pts, 200, 289, f"gate {gate}", gate=gate, min_inlier_fraction=frac)
            assert w["verdict"] == (gate if gate in (2, 3, -1) or frac == 0.0 else MR.LOST)
    # each threshold alone decides
    w = assert_raw_is(ctx, xyz, pts, 200, 289, "min_valid", min_valid=199)
    assert w["n_valid"] == 198 and w["verdict"] == MR.LOST
    assert assert_raw_is(ctx, xyz, pts, 200, 289, "min_valid", min_valid=198)["verdict"] == 0
    err = w["matching_error"]
    assert assert_raw_is(ctx, xyz, pts, 200, 289, "max_error", max_error=err)["verdict"] == 0
    assert assert_raw_is(ctx, xyz, pts, 200, 289, "max_error", max_error=float(np.nextafter(err, 0.0)))["verdict"] == MR.LOST
    frac = w["inlier_fraction"]
    assert assert_raw_is(ctx, xyz, pts, 200, 289, "fraction", min_inlier_fraction=frac)["verdict"] == 0
    assert assert_raw_is(ctx, xyz, pts, 200, 289, "fraction", min_inlier_fraction=float(np.nextafter(frac, 1.0)))["verdict"] == MR.LOST
    # a smaller max_distance than the cell
    w = assert_raw_is(ctx, xyz, pts, 289, 289, "max_distance 0.125", max_distance=0.125)
    assert 0 < w["n_inliers"] < assert_raw_is(ctx, xyz, pts, 289, 289)["n_inliers"]
    # max_range exactly on a point's range: (0.75, 1, 0) is 1.25 from the sensor, (0.75, 1, 1/64) is further
    rp = np.array([[0.75, 1.0, 0.0], [0.75, 1.0, 0.015625], [-1.25, 0.0, 0.0], [0.0, 0.0, np.nextafter(1.25, 2.0)]])
    w = assert_raw_is(ctx, xyz, rp, 4, 4, "max_range", max_range=1.25)
    assert (w["d2"] >= 0).tolist() == [True, False, True, False] and w["n_valid"] == 2
    assert assert_raw_is(ctx, xyz, rp, 4, 4, "max_range 0", max_range=0.0)["n_valid"] == 0
    assert assert_raw_is(ctx, xyz, rp, 4, 4, "max_range inf", max_range=math.inf)["n_valid"] == 4
    ctx.check_errors(stream())


def test_an_empty_map_has_no_inliers(lattice_points):
    ctx = new_context(np.zeros((0, 3)), 0.5)
    want = MR.status(lattice_points, 100, 289, T_LATTICE, np.zeros((0, 3)), 0.5)
    out, d2 = raw_status(ctx, lattice_points, 100, 289, T_LATTICE)
    assert out == MR.out_bytes(want) and d2[:100].tobytes() == want["d2"].tobytes()
    assert (want["n_valid"], want["n_inliers"], want["matching_error"], want["verdict"]) == (98, 0, math.inf, 0)
    ctx.check_errors(stream())


def test_the_raw_call_refuses_what_the_header_says(lattice, lattice_points):
    from sps_amd import _native
    ctx, xyz = lattice
    pts = lattice_points
    for kw in (dict(max_distance=0.5000001), dict(max_distance=0.0), dict(max_distance=math.inf), dict(max_distance=math.nan),
               dict(max_range=math.nan), dict(min_inlier_fraction=math.nan), dict(max_error=math.nan), dict(min_valid=-1)):
        with pytest.raises(_native.SpsError):
            raw_status(ctx, pts, 10, 289, T_LATTICE, **kw)
    with pytest.raises(_native.SpsError):
        raw_status(_native.Context(0), pts, 10, 289, T_LATTICE)            # no grid was uploaded
    # cap beyond SPS_MAX_POINTS = 2^23: refused before any launch, so small buffers do
    too_many = (1 << 23) + 1
    assert _native.lib.sps_loc_match_status_scratch(too_many) == -1 and _native.lib.sps_loc_match_status_scratch(1 << 23) > 0
    small = torch.zeros(64, dtype=torch.float64, device="cuda")
    n_dev = torch.tensor([10], dtype=torch.int32, device="cuda")
    args = (dev(T_LATTICE.reshape(16)).data_ptr(), None, 0.5, -1.0, 0.0, math.inf, 1, small.data_ptr(), None, small.data_ptr() + 64)
    with pytest.raises(_native.SpsError):
        ctx.loc_match_status(small.data_ptr() + 256, n_dev.data_ptr(), too_many, *args, stream())
    with pytest.raises(_native.SpsError):
        ctx.loc_match_status(small.data_ptr() + 256, n_dev.data_ptr(), -1, *args, stream())
    torch.cuda.synchronize()
    assert not small.any()                                                 # nothing was written
    assert_raw_is(ctx, xyz, pts, 10, 289, "after the refusals")            # none of them left anything behind
    ctx.check_errors(stream())


# ---- the scene ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from scipy.spatial import cKDTree
    scan = sensor_scan(1)
    map_xyz = synthetic.build_map(**KW)[:, :3].astype(np.float64)
    return dict(map=map_xyz, scan=scan, pts=LR.downsample(scan, len(scan), LEAF)[1], tree=cKDTree(map_xyz))


@pytest.fixture(scope="module")
def ndt(scene):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(scene["map"], leaf=LEAF, match_status=OPTS)


def same_match(a, b, verdict=True):
    """two MatchStatus with the same bits (``verdict`` false: but for the gate word that went in)"""
    assert np.float64(a.inlier_fraction).tobytes() == np.float64(b.inlier_fraction).tobytes()
    assert np.float64(a.matching_error).tobytes() == np.float64(b.matching_error).tobytes()
    assert (a.n_valid, a.n_inliers, a.lost) == (b.n_valid, b.n_inliers, b.lost)
    assert not verdict or a.verdict == b.verdict


def match_is(m, want):
    assert (m.n_valid, m.n_inliers, m.verdict) == (want["n_valid"], want["n_inliers"], want["verdict"])
    assert np.float64(m.inlier_fraction).tobytes() == np.float64(want["inlier_fraction"]).tobytes()
    assert np.float64(m.matching_error).tobytes() == np.float64(want["matching_error"]).tobytes()
    assert m.lost == (want["verdict"] == MR.LOST)


def restated(scene, pose, gate=None, cell=0.5, **opts):
    pts = scene["pts"]
    return MR.status(pts, len(pts), len(pts), pose, scene["map"], cell, gate_in=gate, tree=scene["tree"], **dict(OPTS, **opts))


def test_a_good_registration_matches_and_a_kidnapped_one_is_lost(scene, ndt):
    scan = dev(scene["scan"])
    r = ndt(scan, len(scan), T_INIT)
    assert r.status == 0 and r.n_points == len(scene["pts"]) and not r.match.lost and r.ok
    match_is(r.match, restated(scene, r.pose, r.status))                   # the restatement at the device's end pose
    print(f"T_INIT: fraction {r.match.inlier_fraction:.4f} error {r.match.matching_error:.5f}")
    assert r.match.inlier_fraction > THRESHOLD and r.match.verdict == 0
    same_match(ndt(scan, len(scan), T_INIT).match, r.match)                # two calls: the same bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        busy = torch.randn(1 << 20, device="cuda").sort()[0]               # a kernel in front, on the side stream
        pend = ndt.submit(scan, len(scan), T_INIT)
    on_side = pend.result()
    torch.cuda.current_stream().wait_stream(side)
    assert on_side.pose.tobytes() == r.pose.tobytes() and busy.numel() == 1 << 20
    same_match(on_side.match, r.match)
    for T0 in T_KIDNAPPED:
        k = ndt(scan, len(scan), T0)
        print(f"kidnapped: status {k.status} fraction {k.match.inlier_fraction:.4f} error {k.match.matching_error:.5f}")
        assert k.status == 1 and k.match.lost and k.match.verdict == 4 and k.match.inlier_fraction < THRESHOLD
        match_is(k.match, restated(scene, k.pose, k.status))
    ndt.ctx.check_errors(stream())


def test_match_status_at_gives_the_distances(scene, ndt):
    scan = dev(scene["scan"])
    m, d2 = ndt.match_status_at(scan, len(scan), T_TRUE, distances=True).result()
    want = restated(scene, T_TRUE)
    match_is(m, want)
    assert d2.tobytes() == want["d2"].tobytes() and len(d2) == len(scene["pts"])
    same_match(ndt.match_status_at(scan, len(scan), T_TRUE).result(), m)
    with pytest.raises(ValueError):
        ndt.match_status_at(scan, len(scan), np.full((4, 4), np.nan))
    ndt.ctx.check_errors(stream())


def test_the_icp_localiser_takes_the_status_on_its_own_grid(scene):
    from sps_amd.localiser import ScanToMapLocaliser
    with pytest.raises(ValueError):
        ScanToMapLocaliser(scene["map"], max_distance=0.4, leaf=LEAF, match_status=dict(max_distance=0.5))
    with pytest.raises(ValueError):
        ScanToMapLocaliser(scene["map"], leaf=LEAF, match_status=dict(distance=0.5))
    icp = ScanToMapLocaliser(scene["map"], max_distance=1.0, leaf=LEAF, match_status=dict(OPTS, max_range=25.0))
    plain = ScanToMapLocaliser(scene["map"], max_distance=1.0, leaf=LEAF)
    scan = dev(scene["scan"])
    r, p = icp(scan, len(scan), T_INIT), plain(scan, len(scan), T_INIT)
    assert r.pose.tobytes() == p.pose.tobytes() and r.trace.tobytes() == p.trace.tobytes() and p.match is None
    want = restated(scene, r.pose, r.status, cell=1.0, max_range=25.0)     # the ICP's grid has 1 m cells
    match_is(r.match, want)
    assert r.status == 0 and not r.match.lost and 0 < want["n_valid"] < len(scene["pts"])
    k = icp(scan, len(scan), T_KIDNAPPED[0])
    assert k.match.lost or k.status in (2, 3)
    match_is(k.match, restated(scene, k.pose, k.status, cell=1.0, max_range=25.0))
    icp.ctx.check_errors(stream())


# ---- the gate ----------------------------------------------------------------------------------------------------------------
def test_a_lost_frame_leaves_the_online_map_and_the_estimator_alone(scene):
    from sps_amd.localiser import NDTLocaliser
    from sps_amd.pose_estimator import PoseEstimator
    scan = dev(scene["scan"])
    n_cells = NDTLocaliser(scene["map"], leaf=LEAF).n_cells
    dyn = NDTLocaliser(scene["map"], leaf=LEAF, cell_capacity=2 * n_cells, match_status=OPTS)
    plain = NDTLocaliser(scene["map"], leaf=LEAF, cell_capacity=2 * n_cells)
    before, carve_before = dyn.map_cells(), dyn.carve_state()
    est = PoseEstimator(T_KIDNAPPED[0], dyn.device)
    state = est.state_dev.clone()
    pend = dyn.submit(scan, len(scan), T_KIDNAPPED[0], integrate=True, carve=True)
    est.correct_from(pend)
    r = pend.result()
    assert r.status == 1 and r.match.lost                                  # the registration's own status would open the gates
    assert (r.map_update.points, r.map_update.founded, r.map_update.dropped, r.map_carve.rays, r.map_carve.cleared) == (0,) * 5
    for a, b in zip(before + carve_before, dyn.map_cells() + dyn.carve_state()):
        assert a.tobytes() == b.tobytes()
    assert torch.equal(state, est.state_dev)                               # a closed gate: every byte of the state block
    # the same frame without the status is folded in, carved with and corrected with: what the status is there to stop
    est2 = PoseEstimator(T_KIDNAPPED[0], plain.device)
    pend = plain.submit(scan, len(scan), T_KIDNAPPED[0], integrate=True, carve=True)
    est2.correct_from(pend)
    w = pend.result()
    assert w.pose.tobytes() == r.pose.tobytes() and w.map_update.points > 0 and w.map_carve.rays > 0
    assert not torch.equal(state, est2.state_dev)
    # a frame that matches: the map of a localiser without the status, the same results, the estimator corrected
    dyn2 = NDTLocaliser(scene["map"], leaf=LEAF, cell_capacity=2 * n_cells, match_status=OPTS)
    plain2 = NDTLocaliser(scene["map"], leaf=LEAF, cell_capacity=2 * n_cells)
    est3 = PoseEstimator(T_INIT, dyn2.device)
    state3 = est3.state_dev.clone()
    pend = dyn2.submit(scan, len(scan), T_INIT, integrate=True, carve=True)
    est3.correct_from(pend)
    a, b = pend.result(), plain2(scan, len(scan), T_INIT, integrate=True, carve=True)
    assert not a.match.lost and a.pose.tobytes() == b.pose.tobytes()
    assert a.map_update == b.map_update and a.map_carve == b.map_carve and a.map_update.points > 1000
    for x, y in zip(dyn2.map_cells() + dyn2.carve_state(), plain2.map_cells() + plain2.carve_state()):
        assert x.tobytes() == y.tobytes()
    assert not torch.equal(state3, est3.state_dev)
    for loc in (dyn, plain, dyn2, plain2):
        loc.ctx.check_errors(stream())


def test_reset_gives_the_state_of_a_new_estimator():
    from sps_amd.pose_estimator import PoseEstimator
    est = PoseEstimator(T_INIT, "cuda", initial_velocity=(0.3, 0.0, 0.0), initial_cov=0.02)
    est.predict(0.1)
    est.correct(T_TRUE)
    est.predict(0.1)
    fresh = PoseEstimator(T_TRUE, "cuda", initial_velocity=(1.0, -2.0, 0.5), initial_cov=0.02)
    assert not torch.equal(est.state_dev, fresh.state_dev)
    est.reset(T_TRUE, velocity=(1.0, -2.0, 0.5))
    assert torch.equal(est.state_dev, fresh.state_dev) and torch.equal(est.pose_dev, fresh.pose_dev)
    est.predict(0.1)
    fresh.predict(0.1)
    assert torch.equal(est.state_dev, fresh.state_dev) and torch.equal(est.pose_dev, fresh.pose_dev)
    est.reset(T_INIT)
    assert torch.equal(est.state_dev, PoseEstimator(T_INIT, "cuda", initial_cov=0.02).state_dev)
    with pytest.raises(ValueError):
        est.reset(np.full((4, 4), np.inf))


# ---- match_status=None -------------------------------------------------------------------------------------------------------
def test_without_match_status_nothing_changes(scene):
    from sps_amd.localiser import NDTLocaliser, pose_grid
    a = NDTLocaliser(scene["map"], leaf=LEAF, match_status=None)
    b = NDTLocaliser(scene["map"], leaf=LEAF)
    scan = dev(scene["scan"])
    starts = T_INIT @ pose_grid([0.0, 0.5], [0.0], [0.0, 5.0])
    calls = (lambda l: l.submit(scan, len(scan), T_INIT, with_normal=True), lambda l: l.submit_batch(scan, len(scan), starts),
             lambda l: l.relocalise(scan, len(scan), starts, keep=2))
    for call in calls:
        pa, pb = call(a), call(b)
        ra, rb = pa.result(), pb.result()
        assert pa._host.numpy().tobytes() == pb._host.numpy().tobytes()
        assert getattr(pa, "_batch", pa)._layout() == getattr(pb, "_batch", pb)._layout()
        assert getattr(ra, "batch", ra).match is None and getattr(rb, "batch", rb).match is None
    with pytest.raises(ValueError):
        a.match_status_at(scan, len(scan), T_INIT)
    # and with it, the registration itself gives the same bits: the status only follows it
    c = NDTLocaliser(scene["map"], leaf=LEAF, match_status=OPTS)
    ra, rc = a(scan, len(scan), T_INIT, with_normal=True), c(scan, len(scan), T_INIT, with_normal=True)
    assert ra.pose.tobytes() == rc.pose.tobytes() and ra.trace.tobytes() == rc.trace.tobytes()
    assert ra.normal.tobytes() == rc.normal.tobytes() and (ra.status, ra.iterations, ra.n_corr) == (rc.status, rc.iterations, rc.n_corr)
    a.ctx.check_errors(stream())


# ---- every entry point reports the status at the pose it hands on --------------------------------------------------------
def at(loc, scan, pose):
    return loc.match_status_at(scan, len(scan), pose).result()


def test_the_batch_entry_points_report_the_status_at_the_selected_pose(scene, ndt):
    from sps_amd.localiser import pose_grid
    scan = dev(scene["scan"])
    starts = T_INIT @ pose_grid([0.0, 0.5], [0.0], [0.0, 5.0])
    b = ndt.submit_batch(scan, len(scan), starts).result()
    assert b.best >= 0 and not b.match.lost and b.match.verdict == b.results[b.best].status
    same_match(b.match, at(ndt, scan, b.pose), verdict=False)
    d = ndt.submit_from_device(scan, len(scan), dev(T_INIT.reshape(16))).result()
    same_match(d.match, at(ndt, scan, d.pose), verdict=False)
    assert d.pose.tobytes() == ndt(scan, len(scan), T_INIT).pose.tobytes() and not d.match.lost
    s = ndt.relocalise(scan, len(scan), starts, keep=2).result()
    same_match(s.batch.match, at(ndt, scan, s.pose), verdict=False)
    assert s.ok and not s.batch.match.lost
    lost = ndt.submit_batch(scan, len(scan), np.stack(T_KIDNAPPED)).result()   # every hypothesis in a wrong basin
    assert lost.best >= 0 and lost.match.lost and lost.match.verdict == 4
    same_match(lost.match, at(ndt, scan, lost.pose), verdict=False)
    # no hypothesis selected: -1 passes through
    none = ndt.submit_batch(scan[:40], 40, starts).result()
    assert none.best == -1 and none.match.verdict == -1 and not none.match.lost
    ndt.ctx.check_errors(stream())


def test_the_pyramid_and_the_source_cells_report_the_status(scene):
    from sps_amd.localiser import NDTLocaliser
    scan = dev(scene["scan"])
    for kw in (dict(resolutions=(2.0, 1.0)), dict(source="cells")):
        loc = NDTLocaliser(scene["map"], leaf=LEAF, match_status=OPTS, **kw)
        plain = NDTLocaliser(scene["map"], leaf=LEAF, **kw)
        r, p = loc(scan, len(scan), T_INIT), plain(scan, len(scan), T_INIT)
        assert r.pose.tobytes() == p.pose.tobytes() and (r.status, r.iterations, r.n_corr, r.n_sources) == (p.status, p.iterations,
                                                                                                         p.n_corr, p.n_sources)
        assert r.status in (0, 1) and not r.match.lost and r.match.verdict == r.status
        same_match(r.match, at(loc, scan, r.pose), verdict=False)
        match_is(r.match, restated(scene, r.pose, r.status))
        loc.ctx.check_errors(stream())


def test_localise_global_reports_the_status():
    from sps_amd.localiser import NDTLocaliser
    from tests.test_bbs_cpu import CORRIDOR, corridor_scene
    s = corridor_scene()
    loc = NDTLocaliser(s["map_xyz"], resolution=1.0, leaf=0.2, iterations=8, global_grid=CORRIDOR["grid"], match_status=OPTS)
    scan = dev(s["scan"])
    g = loc.localise_global(scan, len(scan), CORRIDOR["yaw_steps"], keep=4, scan_z=CORRIDOR["scan_z"]).result()
    assert g.ok and not g.batch.match.lost
    same_match(g.batch.match, at(loc, scan, g.pose), verdict=False)
    dt, dr = LR.pose_difference(g.pose, s["T_true"])
    print(f"global: {dt:.3f} m {dr:.4f} rad, fraction {g.batch.match.inlier_fraction:.4f}")
    loc.ctx.check_errors(stream())


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def test_the_loop_flags_a_kidnapped_frame_and_recovers_globally():
    """Five frames on the synthetic corridor; from frame 2 on the sensor is turned by 90 degrees against what the loop
    believes: (0, 0, 90) of the table in tests/test_match_status_cpu.py.  A sensor 10 m further along the corridor, the
    kidnap first thought of, does not do: walls and ground look the same there, and the restatements give that frame an
    inlier fraction of 0.95 (registered from frame 1's pose: status 1, 10.7 m off), above the threshold."""
    from scipy.spatial import cKDTree
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser
    from sps_amd.sps_filters import SPSCVMFilter
    n, step = 5, 0.5
    mp = synthetic.sequence_map(n, step, **KW)
    truth, scans = [], []
    for i in range(n):
        world = synthetic.lidar_scan(100 + i, x_offset=step * i, **KW)
        T = LR.perturbation(step * i, 0.0, 0.0, math.degrees(0.02 * i))
        if i >= 2:
            T = T @ LR.perturbation(0.0, 0.0, 0.0, 90.0)
        Ti = np.linalg.inv(T)
        scans.append(np.c_[world[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3], world[:, 3]].astype(np.float32))
        truth.append(T)
    map64 = mp[:, :3].astype(np.float64)
    # what the test rests on, from the restatements: registered from frame 1's pose, frame 2 ends lost
    pts2 = LR.downsample(scans[2], len(scans[2]), LEAF)[1]
    ref = NR.align(pts2, NR.cells(map64, 1.0), truth[1], iters=30)
    frac = MR.status(pts2, len(pts2), len(pts2), ref["pose"], map64, 0.5, tree=cKDTree(map64))["inlier_fraction"]
    print(f"restatement, frame 2: status {ref['status']}, {LR.pose_difference(ref['pose'], truth[2])[1]:.2f} rad off, fraction {frac:.4f}")
    assert ref["status"] in (0, 1) and frac < THRESHOLD

    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(np.ascontiguousarray(mp[:, :3], dtype=np.float32))
    grid = dict(resolution=0.5, map_z=(-1.0, 3.0), levels=3)

    def run(**kw):
        loc = NDTLocaliser(map64, leaf=LEAF, global_grid=grid, **kw.pop("localiser", {}))
        loop = LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0), loc, truth[0], **kw)
        steps = [loop.step(s, **({} if loop.estimator is None else dict(dt=0.1))) for s in scans]
        loc.ctx.check_errors(stream())
        return steps

    steps = run(localiser=dict(match_status=OPTS), recover=dict(after=1, yaw_steps=72, scan_z=(-1.0, 3.0)))
    for i, s in enumerate(steps):
        dt, dr = LR.pose_difference(s.pose, truth[i])
        print(f"frame {i}: flagged {s.flagged} recovered {s.recovered} status {s.pose_result.status} fraction "
              f"{s.match.inlier_fraction:.4f} error {s.match.matching_error:.5f}; {dt:.3f} m {dr:.4f} rad from the truth")
    assert [s.flagged for s in steps] == [False, False, True, False, False]
    assert [s.recovered for s in steps] == [False, False, False, True, False]
    assert steps[2].match.lost and steps[2].pose_result.status in (0, 1)
    assert steps[2].pose.tobytes() == steps[2].guess.tobytes()             # the pose kept
    assert steps[3].global_result.ok and not steps[3].match.lost
    dt, dr = LR.pose_difference(steps[3].pose, truth[3])                   # the global search, then the registration
    assert dt < 0.1 and dr < 0.01
    assert not steps[4].match.lost and LR.pose_difference(steps[4].pose, truth[4])[1] < 0.01
    # without the status the lost frame is handed on, unflagged: what the feature exists to catch
    blind = run()
    dr = LR.pose_difference(blind[2].pose, truth[2])[1]
    print(f"without match_status, frame 2: flagged {blind[2].flagged}, {dr:.2f} rad from the truth")
    assert not blind[2].flagged and dr > 1.0 and blind[2].match is None
    for i in (0, 1):
        assert blind[i].pose.tobytes() == steps[i].pose.tobytes()
    # with an estimator: the lost frame leaves it uncorrected, the recovered pose re-initialises it
    from sps_amd.pose_estimator import PoseEstimator
    est = PoseEstimator(truth[0], "cuda")
    with_est = run(localiser=dict(match_status=OPTS), recover=dict(after=1, yaw_steps=72, scan_z=(-1.0, 3.0)), estimator=est)
    assert [s.flagged for s in with_est] == [False, False, True, False, False]
    assert [s.recovered for s in with_est] == [False, False, False, True, False]
    close = lambda a, b: max(LR.pose_difference(a, b)) < 1e-9              # the same pose through the state's quaternion
    assert close(with_est[2].estimate, with_est[2].guess)                  # uncorrected: still the prediction
    assert LR.pose_difference(with_est[3].pose, truth[3])[0] < 0.1 and with_est[3].estimate.tobytes() == with_est[3].pose.tobytes()
    # the prediction of the re-initialised estimator over 0.1 s at zero velocity: the same position, the heading nearly
    dt, dr = LR.pose_difference(with_est[4].guess, with_est[3].pose)
    print(f"with an estimator, frame 4: the guess is {dt:.2e} m {dr:.2e} rad from frame 3's pose")
    assert dt < 1e-9 and dr < 1e-3
    assert est.state().n_correct == 1                                      # frame 4's, since the reset
    with pytest.raises(ValueError):
        LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0),
                         NDTLocaliser(map64, leaf=LEAF, match_status=OPTS), truth[0], recover=dict(after=1, yaw_steps=72))
