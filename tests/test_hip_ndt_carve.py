"""GPU tests of the online NDT map's free-space carving (sps_amd.localiser.NDTLocaliser.carve, submit(..., carve=True); C ABI:
the "NDT localiser, online map: free-space carving" section of include/sps_hip.h) against the numpy restatement in
tests/ndt_carve_reference.py.  Shapes are those of test_hip_ndt_update.py: the 57 k-point synthetic map plus the phantom pole
of test_ndt_carve_cpu.py (2 535 cells of 1 m), 12.8 k-point scans thinned at leaf 0.4 to ~4.2 k rays.  The carve's results are
integer counts and comparisons of individually rounded doubles, so everything is compared exactly.

The cleared cell's S has no getter of its own; it shows only through a later update, whose stored-n = 0 branch does not read
it, so the refilled cell is compared instead (test_the_combined_call_equals_its_three_parts)."""
import copy

import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from tests import localiser_reference as LR
from tests import ndt_carve_reference as CR
from tests import ndt_reference as NR
from tests import ndt_update_reference as UR
from tests.helpers import CFG, net_from_params
from tests.test_hip_ndt_update import CAPACITY, RES, TOL_FLOOR, assert_map_is, assert_same_cells, dev, make, raw_cells, stream
from tests.test_ndt_carve_cpu import phantom_pole, phantom_scene, tie_rays
from tests.test_ndt_cpu import LEAF, T_INIT, T_TRUE, sensor_scan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    """the map with the phantom pole, the ids of the phantom-only cells and the restatement's map of it (read-only)"""
    with_pole, only = phantom_scene()
    return with_pole, only, UR.build(with_pole, CAPACITY)


@pytest.fixture(scope="module")
def scans():
    """sensor scans 1 .. 4 taken at T_TRUE and their thinned float64 points (read-only)"""
    out = {}
    for seed in (1, 2, 3, 4):
        s = sensor_scan(seed)
        out[seed] = (s, LR.downsample(s, len(s), LEAF)[1])
    return out


@pytest.fixture(scope="module")
def box():
    """8 000 points that fill the 1 000 cells of [-4, 6)^3, eight each: every cell valid, Gaussians about 0.25 m wide"""
    rng = np.random.default_rng(21)
    c = np.stack(np.meshgrid(*[np.arange(-4, 6)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    mp = (c[:, None, :] + 0.1 + 0.8 * rng.random((len(c), 8, 3))).reshape(-1, 3)
    m = UR.build(mp, 1024)
    assert len(m["keys"]) == 1000 and m["valid"].all()
    return mp, m


def raw_carve(loc, pts, n, cap, T, gate=None, T_on_device=False, end_margin=None, through_sigma=1.0, min_pass=2, miss_frames=3,
              max_steps=512):
    """sps_ndt_map_carve itself on float64 points: returns info as a list"""
    buf = np.zeros((max(cap, len(pts), 1), 3))
    buf[:len(pts)] = pts
    p = dev(buf)
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    g = None if gate is None else torch.tensor([gate], dtype=torch.int32, device="cuda")
    Td = dev(np.asarray(T, dtype=np.float64).reshape(16)) if T_on_device else None
    loc.ctx.ndt_map_carve(p.data_ptr(), n_dev.data_ptr(), cap, None if T_on_device else T, Td.data_ptr() if T_on_device else None,
                          g.data_ptr() if g is not None else None, loc.resolution if end_margin is None else end_margin,
                          through_sigma, min_pass, miss_frames, max_steps, info.data_ptr(), None, stream())
    out = [int(v) for v in info.cpu().numpy()]
    loc.ctx.check_errors(stream())
    return out


def info_of(r):
    return [r.rays, r.seen_through, r.cleared, r.cut]


def assert_state_is(loc, m, what=""):
    """pass, hit and miss of every assigned cell, and then the whole map, against the restatement's"""
    for name, got, want in zip(("pass", "hit", "miss"), loc.carve_state(), CR.state(m)):
        np.testing.assert_array_equal(got.astype(np.int64), want, str((what, name)))
    assert_map_is(loc, m, what)


def pose_at(o):
    T = np.eye(4)
    T[:3, 3] = o
    return T


# ---- the test scene ------------------------------------------------------------------------------------------------------
def test_three_frames_match_the_restatement_and_clear_the_phantom(scene, scans):
    with_pole, only, m0 = scene
    m = copy.deepcopy(m0)
    dyn = make(with_pole)
    before = raw_cells(dyn)
    others = np.setdiff1d(np.arange(len(m["keys"])), only)
    for frame in (1, 2, 3):
        scan, pts = scans[frame]
        want = CR.carve(m, pts, T_TRUE)
        got = dyn.carve(dev(scan), len(scan), T_TRUE).result()
        print(f"frame {frame}: info (rays, seen through, cleared, cut) {want}; cells with a pass {int((m['pass'] > 0).sum())}, "
              f"with a hit {int((m['hit'] > 0).sum())}")
        assert info_of(got) == want and got.n_points == len(pts) == want[0]
        assert want[1] == 2 and want[2] == (2 if frame == 3 else 0) and (m["pass"] > 0).sum() > 2 and (m["hit"] > 0).sum() > 500
        assert_state_is(dyn, m, frame)
    after = raw_cells(dyn)
    assert (after["count"][only] == 0).all() and not after["valid"][only].any() and not after["mean"][only].any()
    assert (after["keys"][only] == before["keys"][only]).all()                  # a cleared cell keeps its key and its id
    keep = np.ones(CAPACITY, dtype=bool)
    keep[only] = False
    assert_same_cells({k: after[k][keep] for k in after}, {k: before[k][keep] for k in before})   # every other cell keeps every bit
    assert len(others) == 2533 and dyn.map_info() == (2535, CAPACITY, 0)
    # a cleared cell that receives points again has the bits of a founded cell: the update's stored-n = 0 branch
    pole = LR.transform(phantom_pole()[:40], np.linalg.inv(T_TRUE))
    rows = np.concatenate([scans[4][0], np.c_[pole, np.zeros(len(pole))].astype(np.float32)])
    pts = LR.downsample(rows, len(rows), LEAF)[1]
    want = UR.update(m, pts, T_TRUE)
    u = dyn.integrate(dev(rows), len(rows), T_TRUE).result()
    assert [u.cells, u.founded, u.dropped, u.points] == want and (m["count"][only] > 0).all()
    assert_state_is(dyn, m, "refilled")
    dyn.ctx.check_errors(stream())


# ---- edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 300, 400])
def test_ray_counts(box, n):
    """300 rays from inside the box of valid cells; cap = 300 rows: 300 is the cap itself, 400 a device count above it"""
    mp, m0 = box
    m = copy.deepcopy(m0)
    rng = np.random.default_rng(4)
    v = rng.normal(size=(300, 3))
    pts = v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(2.0, 4.5, 300)[:, None]
    T = pose_at((1.3, 0.9, 1.6))
    dyn = make(mp, capacity=1024)
    kw = dict(min_pass=1, miss_frames=2)
    assert raw_carve(dyn, pts, n, 300, T, **kw) == CR.carve(m, pts, T, cap=300, n=n, **kw)
    assert_state_is(dyn, m, n)
    # once more with the pose on the device: the same cells are seen through again, and cleared
    want = CR.carve(m, pts, T, cap=300, n=n, **kw)
    assert raw_carve(dyn, pts, n, 300, T, T_on_device=True, **kw) == want and want[0] == min(n, 300)
    assert want[2] == want[1] and (want[2] > 0 or n == 0)
    assert_state_is(dyn, m, n)


def test_bad_rays_and_tie_rays(box):
    mp, m0 = box
    m = copy.deepcopy(m0)
    dyn = make(mp, capacity=1024)
    kw = dict(min_pass=1, miss_frames=100)
    passes = 0
    for name, o, q, margin, max_steps, cells, cut in tie_rays():
        p = (np.asarray(q) - np.asarray(o))[None]                              # exact: every number is dyadic
        want = CR.carve(m, p, pose_at(o), end_margin=margin, max_steps=max_steps, **kw)
        assert raw_carve(dyn, p, 1, 1, pose_at(o), end_margin=margin, max_steps=max_steps, **kw) == want, name
        assert want[0] == 1 and want[3] == int(cut) and m["hit"].sum() == 1, name
        assert m["pass"].sum() <= len(cells), name
        passes += int(m["pass"].sum())
        assert_state_is(dyn, m, name)
    assert passes > 10
    bad = np.array([[1.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [2.0e6, 0.0, 0.0], [0.0, 0.0, -3.0], [0.0, -np.inf, 1.0]])
    want = CR.carve(m, bad, pose_at((0.5, 0.5, 0.5)), **kw)
    assert raw_carve(dyn, bad, len(bad), len(bad), pose_at((0.5, 0.5, 0.5)), **kw) == want and want[0] == 2
    assert_state_is(dyn, m, "bad rows")
    far = pose_at((2.0e6, 0.5, 0.5))                                           # the sensor beyond the key range: nothing is cast
    want = CR.carve(m, bad, far, **kw)
    assert raw_carve(dyn, bad, len(bad), len(bad), far, **kw) == want == [0, 0, 0, 0]
    assert_state_is(dyn, m, "far sensor")
    dyn.ctx.check_errors(stream())


# ---- determinism ---------------------------------------------------------------------------------------------------------
def test_a_permutation_and_a_second_run_give_the_same_bits(scene, scans):
    with_pole, _, _ = scene
    pts = scans[2][1]
    perm = np.random.default_rng(9).permutation(len(pts))
    kw = dict(min_pass=1, miss_frames=2, through_sigma=2.0)
    out = []
    for order in (None, None, perm):
        dyn = make(with_pole)
        p = pts if order is None else pts[order]
        infos = [raw_carve(dyn, p, len(p), len(p), T_TRUE, **kw) for _ in range(2)]
        out.append((infos, dyn.carve_state(), raw_cells(dyn)))
    assert out[0][0][1][2] > 0                                                 # cells were cleared
    for infos, state, cells in out[1:]:
        assert infos == out[0][0]
        for a, b in zip(state, out[0][1]):
            assert a.tobytes() == b.tobytes()
        assert_same_cells(cells, out[0][2])


# ---- the gate ------------------------------------------------------------------------------------------------------------
def test_the_gate_follows_the_status_on_the_device(scene, scans):
    with_pole, _, _ = scene
    scan, pts = scans[1]
    closed = make(with_pole, min_correspondences=len(pts) + 1)
    first = closed.carve(dev(scan), len(scan), T_TRUE).result()                # state worth keeping
    assert first.rays == len(pts) and first.seen_through == 2
    before, state = raw_cells(closed), closed.carve_state()
    assert state[0].any() and state[1].any() and state[2].any()
    s2 = dev(scans[2][0])
    r = closed.submit(s2, len(s2), T_INIT, carve=True, carve_options=dict(min_pass=1, miss_frames=1)).result()
    assert r.status == 2 and info_of(r.map_carve) == [0, 0, 0, 0] and r.map_update is None
    b = closed.submit_batch(s2, len(s2), np.stack([T_INIT, T_TRUE]), carve=True, integrate=True,
                            carve_options=dict(min_pass=1, miss_frames=1)).result()
    assert b.best == -1 and info_of(b.map_carve) == [0, 0, 0, 0] and b.map_update.points == 0
    assert raw_carve(closed, pts, len(pts), len(pts), T_TRUE, gate=3, min_pass=1, miss_frames=1) == [0, 0, 0, 0]
    assert_same_cells(raw_cells(closed), before)
    for a, b_ in zip(closed.carve_state(), state):
        assert a.tobytes() == b_.tobytes()
    assert closed.submit(s2, len(s2), T_INIT).result().map_carve is None
    closed.ctx.check_errors(stream())


def test_the_combined_call_equals_its_three_parts(scene, scans):
    """carve, then update (min_pass = 1 and miss_frames = 1: one frame clears)"""
    with_pole, _, m0 = scene
    scan, pts = scans[1]
    opts = dict(min_pass=1, miss_frames=1, through_sigma=2.0)
    one, parts = make(with_pole), make(with_pole)
    r = one.submit(dev(scan), len(scan), T_INIT, integrate=True, carve=True, carve_options=opts).result()
    p = parts.submit(dev(scan), len(scan), T_INIT).result()
    assert r.status == p.status == 0 and r.pose.tobytes() == p.pose.tobytes() and p.map_carve is None
    c = parts.carve(dev(scan), len(scan), p.pose, **opts).result()
    u = parts.integrate(dev(scan), len(scan), p.pose).result()
    assert info_of(r.map_carve) == info_of(c) and c.cleared > 0
    assert (r.map_update.cells, r.map_update.founded, r.map_update.dropped, r.map_update.points) == (u.cells, u.founded, u.dropped, u.points)
    assert_same_cells(raw_cells(one), raw_cells(parts))
    for a, b in zip(one.carve_state(), parts.carve_state()):
        assert a.tobytes() == b.tobytes()
    # and both are the restatement's carve followed by its update, at the pose the device found
    m = copy.deepcopy(m0)
    cleared_then = CR.carve(m, pts, r.pose, gate=r.status, **opts)
    assert cleared_then == info_of(c) and (m["count"] == 0).sum() == c.cleared
    UR.update(m, pts, r.pose, gate=r.status)
    assert_state_is(one, m)
    # the same through a batch and through a relocalisation
    from sps_amd.localiser import pose_grid
    for call in ("batch", "search"):
        loc = make(with_pole)
        m = copy.deepcopy(m0)
        if call == "batch":
            b = loc.submit_batch(dev(scan), len(scan), np.stack([T_INIT, T_TRUE]), integrate=True, carve=True, carve_options=opts).result()
        else:
            b = loc.relocalise(dev(scan), len(scan), T_INIT @ pose_grid([0.0, 1.0], [0.0], [-10.0, 0.0, 10.0])[:5], keep=2,
                               integrate=True, carve=True, carve_options=opts).result()
        assert (b.best if call == "batch" else b.batch.best) >= 0
        assert info_of(b.map_carve) == CR.carve(m, pts, b.pose, **opts)
        u = b.map_update
        assert [u.cells, u.founded, u.dropped, u.points] == UR.update(m, pts, b.pose)
        assert_state_is(loc, m, call)
    one.ctx.check_errors(stream())


# ---- stream order --------------------------------------------------------------------------------------------------------
def test_an_alignment_behind_a_carve_on_a_side_stream_sees_the_carved_map(scene, scans):
    with_pole, _, m0 = scene
    dyn = make(with_pole)
    s1, s2 = dev(scans[1][0]), dev(scans[2][0])
    opts = dict(min_pass=1, miss_frames=1)
    T_off = LR.perturbation(0.0, 2.0, 0.0, 25.0) @ T_TRUE                      # a wrong pose: the rays go through walls
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pa = dyn.carve(s1, len(s1), T_off, **opts)
        pb = dyn.submit(s2, len(s2), T_INIT)                                   # no synchronisation in between
    a, b = pa.result(), pb.result()
    m = copy.deepcopy(m0)
    plain = NR.align(scans[2][1], UR.as_cmap(m), T_INIT)
    assert info_of(a) == CR.carve(m, scans[1][1], T_off, **opts) and a.cleared > 100
    fwd = NR.align(scans[2][1], UR.as_cmap(m), T_INIT)
    rev = NR.align(scans[2][1], UR.as_cmap(m), T_INIT, reverse=True)
    spread_t, spread_r = LR.pose_difference(fwd["pose"], rev["pose"])
    tol_t, tol_r = max(100.0 * spread_t, TOL_FLOOR), max(100.0 * spread_r, TOL_FLOOR)
    dt, dr = LR.pose_difference(b.pose, fwd["pose"])
    print(f"cleared {a.cleared}; spread {spread_t:.3e} m {spread_r:.3e} rad; device vs restatement {dt:.3e} m {dr:.3e} rad; "
          f"counted {b.n_corr} (without the carve {plain['n_corr']})")
    assert fwd["faces"] == 0 and fwd["boundary"] == 0
    assert (b.status, b.iterations) == (fwd["status"], fwd["iterations"])
    np.testing.assert_array_equal(b.trace[:, 0], fwd["trace"][:, 0])
    assert dt <= tol_t and dr <= tol_r
    assert fwd["trace"][0, 0] < plain["trace"][0, 0]                           # the carve shows in the first iteration's count
    assert_state_is(dyn, m)


# ---- the loop ------------------------------------------------------------------------------------------------------------
class Recording:
    """the device localiser behind the interface LocalisationLoop uses, keeping every frame's kept rows and guess"""

    def __init__(self, loc):
        self.loc, self.device, self.cell_capacity, self.frames = loc, loc.device, loc.cell_capacity, []

    def submit_filtered(self, pending, T_init, **kw):
        n = int(pending.count_dev.item())
        self.frames.append((pending._filtered[:n].cpu().numpy(), np.array(T_init, dtype=np.float64), kw))
        return self.loc.submit_filtered(pending, T_init, **kw)


def test_the_loop_forgets_the_phantom(scene, scans):
    """Four frames through LocalisationLoop(update_map=True, carve_map=True).  The restatement-driven loop registers every
    frame on its own map (status, iterations and counts equal, the pose within 100 x the forward / reversed spread) and then
    carves and updates that map at the pose the device returned: a pose that differs in its last bits puts other bits into
    the map, so this is the one input the two loops must share for their maps to be compared bit for bit."""
    from sps_amd.localiser import LocalisationLoop
    from sps_amd.sps_filters import SPSCVMFilter
    with_pole, only, m0 = scene
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(np.ascontiguousarray(with_pole, dtype=np.float32))
    like = make(with_pole)
    rec = Recording(like)
    f = SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0)     # every point passes
    loop = LocalisationLoop(f, rec, T_INIT, update_map=True, carve_map=True)
    got = [loop.step(scans[k][0]) for k in (1, 2, 3, 4)]
    m = copy.deepcopy(m0)
    fwd = NR.align(scans[1][1], UR.as_cmap(m), T_INIT)
    rev = NR.align(scans[1][1], UR.as_cmap(m), T_INIT, reverse=True)
    spread_t, spread_r = LR.pose_difference(fwd["pose"], rev["pose"])
    tol_t, tol_r = max(100.0 * spread_t, TOL_FLOOR), max(100.0 * spread_r, TOL_FLOOR)
    for i, step in enumerate(got):
        rows, guess, kw = rec.frames[i]
        a = step.pose_result
        assert kw["carve"] and kw["integrate"] and a.status in (0, 1) and not step.flagged, i
        _, pts = LR.downsample(rows, len(rows), like.leaf, like.capacity)
        r = NR.align(pts, UR.as_cmap(m), guess, like.iterations, like.neighbours, like.min_correspondences, like.outlier_ratio,
                     like.tol_t, like.tol_r)
        dt, dr = LR.pose_difference(a.pose, r["pose"])
        want_c = CR.carve(m, pts, a.pose, gate=a.status)
        want_u = UR.update(m, pts, a.pose, gate=a.status)
        print(f"frame {i}: status {a.status}/{r['status']} iterations {a.iterations}/{r['iterations']} count {a.n_corr}/{r['n_corr']} "
              f"device vs restatement {dt:.3e} m {dr:.3e} rad; carve {a.map_carve}; update {a.map_update}")
        assert (a.status, a.iterations, a.n_corr, a.n_points) == (r["status"], r["iterations"], r["n_corr"], len(pts)), i
        assert dt <= tol_t and dr <= tol_r, i
        assert info_of(a.map_carve) == want_c, i
        u = a.map_update
        assert [u.cells, u.founded, u.dropped, u.points] == want_u, i
    assert (m["count"][only] == 0).all()
    assert_state_is(like, m)
    assert (raw_cells(like)["count"][only] == 0).all()
    like.ctx.check_errors(stream())


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_errors(scene, scans):
    from sps_amd import _native
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser
    with_pole, _, _ = scene
    scan = dev(scans[1][0])
    static = NDTLocaliser(with_pole, resolution=RES, leaf=LEAF)
    pyramid = NDTLocaliser(with_pole, resolution=RES, leaf=LEAF, resolutions=(2.0, 1.0))
    for loc in (static, pyramid):
        with pytest.raises(ValueError):
            loc.carve(scan, len(scan), T_TRUE)
        with pytest.raises(ValueError):
            loc.submit(scan, len(scan), T_INIT, carve=True)
        with pytest.raises(ValueError):
            loc.submit_batch(scan, len(scan), T_INIT[None], carve=True)
        with pytest.raises(ValueError):
            loc.relocalise(scan, len(scan), T_INIT[None], keep=1, carve=True)
        with pytest.raises(ValueError):
            loc.carve_state()
    with pytest.raises(ValueError):
        LocalisationLoop(None, static, T_INIT, carve_map=True)
    dyn = make(with_pole)
    before, state = raw_cells(dyn), dyn.carve_state()
    for bad in (dict(through_sigma=0.0), dict(through_sigma=float("nan")), dict(end_margin=-1.0), dict(end_margin=float("inf")),
                dict(min_pass=0), dict(miss_frames=0), dict(max_steps=0), dict(max_steps=4097)):
        with pytest.raises(ValueError):
            dyn.carve(scan, len(scan), T_TRUE, **bad)
        with pytest.raises(ValueError):
            dyn.submit(scan, len(scan), T_INIT, carve=True, carve_options=bad)
        with pytest.raises(_native.SpsError) as e:                             # and the C ABI checks for itself
            raw_carve(dyn, scans[1][1][:10], 10, 10, T_TRUE, **bad)
        assert e.value.code == _native.ERR_INVALID
    with pytest.raises(ValueError):
        dyn.submit(scan, len(scan), T_INIT, carve=True, carve_options=dict(sigma=1.0))
    with pytest.raises(ValueError):
        dyn.submit(scan, len(scan), T_INIT, carve_options=dict(min_pass=1))
    with pytest.raises(ValueError):
        dyn.carve(scan, len(scan), np.full((4, 4), np.nan))
    with pytest.raises(_native.SpsError) as e:                                 # the C ABI refuses a static map
        raw_carve(static, scans[1][1][:10], 10, 10, T_TRUE)
    assert e.value.code == _native.ERR_INVALID
    with pytest.raises(_native.SpsError):
        static.ctx.ndt_map_carve_cells(None, None, None)
    assert _native.lib.sps_ndt_map_carve_scratch(65537) == -1 and _native.lib.sps_ndt_map_carve_scratch(-1) == -1
    assert _native.lib.sps_ndt_map_carve_scratch(65536) == 0 and _native.lib.sps_version() == 202
    assert_same_cells(raw_cells(dyn), before)                                  # no refused call touched the map
    for a, b in zip(dyn.carve_state(), state):
        assert a.tobytes() == b.tobytes() and not a.any()
    dyn.ctx.check_errors(stream())
