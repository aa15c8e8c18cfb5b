"""GPU tests of the online NDT pyramid (sps_amd.localiser.NDTLocaliser(..., resolutions=..., level_capacities=...); C ABI: the
"NDT localiser, online pyramid" section of include/sps_hip.h).  Every level is compared, bit for bit, with the single online
map of its resolution and capacity driven through the same calls (sps_ndt_map_update / sps_ndt_map_carve), and with the numpy
restatement in tests/ndt_online_pyramid_reference.py, which composes the single map's restatements.  Shapes are those of
test_hip_ndt_update.py: the 57 k-point synthetic map, 12.8 k-point scans thinned at leaf 0.4 to ~4.2 k points.  The update has no
exp and no open sum order and the carve only counts, so maps, counters and info words are compared exactly; only poses that
come out of an alignment are compared under the project's rule, 100 x the restatement's forward / reversed spread."""
import copy

import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_carve_reference as CR
from tests import ndt_online_pyramid_reference as OP
from tests import ndt_reference as NR
from tests import ndt_update_reference as UR
from tests.helpers import CFG, net_from_params
from tests.test_hip_ndt_update import FIELDS, assert_same_cells, dev, raw_cells, stream
from tests.test_ndt_carve_cpu import tie_rays
from tests.test_ndt_cpu import KW, LEAF, T_INIT, T_TRUE, sensor_scan
from tests.test_ndt_online_pyramid_cpu import CAPACITIES, PHANTOM_CELLS, PHANTOM_INFO, RESOLUTIONS, phantom_pyramid_scene
from tests.test_ndt_update_cpu import changed_scene, hand_points

pytestmark = pytest.mark.gpu

TOL_FLOOR = 1e-12
LEVEL_ITERS = (10, 10, 10)


def make(map_xyz, resolutions=RESOLUTIONS, caps=CAPACITIES, **kw):
    from sps_amd.localiser import NDTLocaliser
    kw.setdefault("iterations", 30)
    kw.setdefault("level_iterations", LEVEL_ITERS[:len(resolutions)])
    return NDTLocaliser(map_xyz, resolutions=resolutions, leaf=LEAF, level_capacities=caps, **kw)


def make_singles(map_xyz, resolutions=RESOLUTIONS, caps=CAPACITIES, **kw):
    """the way the parent offers: one online single-map localiser per level"""
    from sps_amd.localiser import NDTLocaliser
    return [NDTLocaliser(map_xyz, resolution=r, leaf=LEAF, cell_capacity=c, **kw) for r, c in zip(resolutions, caps)]


def raw_level(loc, l):
    """sps_ndt_pyramid_cells itself: every row of the level's capacity"""
    C = loc.level_capacities[l]
    key = torch.zeros(C, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(C, dtype=torch.int32, device="cuda")
    mean = torch.zeros((C, 3), dtype=torch.float64, device="cuda")
    icov = torch.zeros((C, 6), dtype=torch.float64, device="cuda")
    valid = torch.zeros(C, dtype=torch.int32, device="cuda")
    loc.ctx.ndt_pyramid_cells(l, key.data_ptr(), cnt.data_ptr(), mean.data_ptr(), icov.data_ptr(), valid.data_ptr())
    return dict(keys=key.cpu().numpy().view(np.uint64), count=cnt.cpu().numpy(), mean=mean.cpu().numpy(), icov=icov.cpu().numpy(),
                valid=valid.cpu().numpy().astype(bool))


def assert_levels_are_singles(pyr, singles, what=""):
    """every level against the single online map of its resolution: all rows of the capacity, the state, the carve counters"""
    for l, one in enumerate(singles):
        assert_same_cells(raw_level(pyr, l), raw_cells(one), (what, l))
        assert pyr.pyramid_info(l) == one.map_info(), (what, l)
        for a, b in zip(pyr.carve_state(l), one.carve_state()):
            assert a.tobytes() == b.tobytes(), (what, l)


def assert_levels_are(pyr, levels, what=""):
    """every level against the restatement's map: the assigned cells in id order, the rest of the capacity empty, the state,
    pass / hit / miss"""
    for l, m in enumerate(levels):
        assert_same_cells(dict(zip(FIELDS, pyr.pyramid_cells(l))), m, (what, l))
        assert_same_cells(raw_level(pyr, l), UR.rows_by_capacity(m), (what, l))
        assert pyr.pyramid_info(l) == (len(m["keys"]), m["capacity"], m["dropped"]), (what, l)
        for name, got, want in zip(("pass", "hit", "miss"), pyr.carve_state(l), CR.state(m)):
            np.testing.assert_array_equal(got.astype(np.int64), want, str((what, l, name)))


def _points(pts, cap):
    buf = np.zeros((max(cap, len(pts), 1), 3))
    buf[:len(pts)] = pts
    return dev(buf)


def raw_update(loc, pts, n, cap, T, gate_ptr=None, max_cell_points=0, T_on_device=False):
    """sps_ndt_pyramid_update itself on float64 points: the info words of every level"""
    from sps_amd import _native
    L = len(loc.resolutions)
    p = _points(pts, cap)
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    info = torch.full((L, 4), -7, dtype=torch.int32, device="cuda")
    scratch = torch.empty(_native.lib.sps_ndt_pyramid_update_scratch(cap, L), dtype=torch.uint8, device="cuda")
    Td = dev(np.asarray(T, dtype=np.float64).reshape(16)) if T_on_device else None
    loc.ctx.ndt_pyramid_update(p.data_ptr(), n_dev.data_ptr(), cap, None if T_on_device else T, Td.data_ptr() if T_on_device else None,
                               gate_ptr, max_cell_points, info.data_ptr(), scratch.data_ptr(), stream())
    out = [[int(v) for v in row] for row in info.cpu().numpy()]
    loc.ctx.check_errors(stream())                                             # never a sticky error
    return out


def raw_carve(loc, pts, n, cap, T, gate_ptr=None, T_on_device=False, end_margin=None, through_sigma=1.0, min_pass=2, miss_frames=3,
              max_steps=512):
    """sps_ndt_pyramid_carve itself on float64 points: the info words of every level"""
    L = len(loc.resolutions)
    p = _points(pts, cap)
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    info = torch.full((L, 4), -7, dtype=torch.int32, device="cuda")
    Td = dev(np.asarray(T, dtype=np.float64).reshape(16)) if T_on_device else None
    em = loc.resolutions if end_margin is None else end_margin
    loc.ctx.ndt_pyramid_carve(p.data_ptr(), n_dev.data_ptr(), cap, None if T_on_device else T, Td.data_ptr() if T_on_device else None,
                              gate_ptr, em, through_sigma, min_pass, miss_frames, max_steps, info.data_ptr(), None, stream())
    out = [[int(v) for v in row] for row in info.cpu().numpy()]
    loc.ctx.check_errors(stream())
    return out


def upd_words(results):
    return [[u.cells, u.founded, u.dropped, u.points] for u in results]


def carve_words(results):
    return [[c.rays, c.seen_through, c.cleared, c.cut] for c in results]


def same_bits(a, b):
    assert (a.status, a.iterations, a.n_corr, a.n_points) == (b.status, b.iterations, b.n_corr, b.n_points)
    for x, y in ((a.pose, b.pose), (a.trace, b.trace), (a.normal, b.normal), (a.levels, b.levels)):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()


def pose_at(o):
    T = np.eye(4)
    T[:3, 3] = o
    return T


@pytest.fixture(scope="module")
def map_xyz():
    return synthetic.build_map(**KW)[:, :3].astype(np.float64)


@pytest.fixture(scope="module")
def scans():
    """sensor scans 1 .. 4 taken at T_TRUE and their thinned float64 points (read-only)"""
    out = {}
    for seed in (1, 2, 3, 4):
        s = sensor_scan(seed)
        out[seed] = (s, LR.downsample(s, len(s), LEAF)[1])
    return out


@pytest.fixture(scope="module")
def levels0(map_xyz):
    """the restatement's levels of the test map (read-only: copy before use)"""
    return OP.build(map_xyz, RESOLUTIONS, CAPACITIES)


@pytest.fixture(scope="module")
def phantom():
    """the phantom scene, per level the ids of the phantom-only cells, the restatement's levels of it (read-only)"""
    with_pole, only = phantom_pyramid_scene()
    return with_pole, only, OP.build(with_pole, RESOLUTIONS, CAPACITIES)


# ---- the build and the alignment -----------------------------------------------------------------------------------------
def test_a_fresh_dynamic_pyramid_is_the_single_dynamic_maps_and_aligns_as_the_static_pyramid(map_xyz, levels0, scans):
    from sps_amd.localiser import NDTLocaliser
    pyr = make(map_xyz)
    assert_levels_are_singles(pyr, make_singles(map_xyz), "build")
    assert_levels_are(pyr, levels0, "build")
    for l, m in enumerate(levels0):
        raw, n = raw_level(pyr, l), len(m["keys"])
        assert len(raw["keys"]) == CAPACITIES[l] > n == pyr.level_cells[l] and (raw["keys"][n:] == UR.EMPTY_KEY).all()
        assert not raw["count"][n:].any() and not raw["mean"][n:].any() and not raw["icov"][n:].any() and not raw["valid"][n:].any()
        assert not any(a.any() for a in pyr.carve_state(l))
    # the alignment runs unchanged on dynamic levels
    static = NDTLocaliser(map_xyz, resolutions=RESOLUTIONS, leaf=LEAF, iterations=30, level_iterations=LEVEL_ITERS)
    scan = dev(scans[1][0])
    T_start = LR.perturbation(0.5, 0.0, 0.0, 0.0) @ T_TRUE
    a, b = static(scan, len(scan), T_start, with_normal=True), pyr(scan, len(scan), T_start, with_normal=True)
    assert a.status in (0, 1) and len(set(a.levels)) == 3 and b.map_update is None and b.map_carve is None
    same_bits(a, b)
    # the single map beside the pyramid is static and untouched
    for g, w in zip(pyr.map_cells(), NDTLocaliser(map_xyz, leaf=LEAF).map_cells()):
        assert g.tobytes() == w.tobytes()
    with pytest.raises(ValueError):
        pyr.map_info()
    with pytest.raises(ValueError):
        pyr.submit_batch(scan, len(scan), T_INIT[None], integrate=True)
    with pytest.raises(ValueError):
        pyr.relocalise(scan, len(scan), T_INIT[None], keep=1, carve=True)
    pyr.ctx.check_errors(stream())


# ---- the update ----------------------------------------------------------------------------------------------------------
def test_one_update_then_three_more_match_the_single_maps_and_the_restatement(map_xyz, levels0, scans):
    pyr, singles = make(map_xyz), make_singles(map_xyz)
    levels = copy.deepcopy(levels0)
    n0 = [len(m["keys"]) for m in levels]
    frames = [(1, 9.0, 0), (2, 9.0, 0), (3, 4.0, 40), (4, 0.0, 40)]            # the first: 9 m to the side, existing and new cells
    for i, (seed, dy, mcp) in enumerate(frames):
        scan, pts = scans[seed]
        T = LR.perturbation(0.0, dy, 0.0, 0.0) @ T_TRUE
        want = OP.update(levels, pts, T, max_cell_points=mcp)
        got = pyr.integrate(dev(scan), len(scan), T, max_cell_points=mcp).result()
        one = [s.integrate(dev(scan), len(scan), T, max_cell_points=mcp).result() for s in singles]
        print(f"update {i}: info per level (cells, founded, dropped, points) {want}")
        assert isinstance(got, tuple) and upd_words(got) == upd_words(one) == want
        assert all(u.n_points == len(pts) for u in got)
        assert_levels_are_singles(pyr, singles, i)
        assert_levels_are(pyr, levels, i)
        if i == 0:
            assert all(w[1] > 50 for w in want) and want[2][1] > want[1][1] > want[0][1]
            assert all((m["count"][:n] != m0["count"]).sum() > 50 for m, m0, n in zip(levels, levels0, n0))
    assert all(m["count"].max() > 40 for m in levels)                         # forgetting had something to bite on
    assert levels[1]["dropped"] > 0 == levels[0]["dropped"] == levels[2]["dropped"]   # and the 1 m level ran out of room alone
    pyr.ctx.check_errors(stream())


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 400])
def test_edge_counts(scans, n):
    """cap = 300 rows; 400 is a device count above it"""
    pts = scans[3][1][:300]
    caps = (512, 512, 512)
    pyr = make(np.zeros((0, 3)), caps=caps)
    levels = OP.build(np.zeros((0, 3)), RESOLUTIONS, caps)
    assert raw_update(pyr, pts, n, 300, T_TRUE) == OP.update(levels, pts, T_TRUE, cap=300, n=n)
    assert_levels_are(pyr, levels, n)
    # once more on the cells that now exist, with the pose on the device
    want = OP.update(levels, pts, T_TRUE, cap=300, n=n)
    assert raw_update(pyr, pts, n, 300, T_TRUE, T_on_device=True) == want and all(w[3] == min(n, 300) and w[1] == 0 for w in want)
    assert_levels_are(pyr, levels, n)
    want = OP.carve(levels, pts, T_TRUE, cap=300, n=n, min_pass=1, miss_frames=1)
    assert raw_carve(pyr, pts, n, 300, T_TRUE, min_pass=1, miss_frames=1) == want and all(w[0] == min(n, 300) for w in want)
    assert_levels_are(pyr, levels, n)


def test_the_capacity_rule_holds_per_level():
    """hand_points found four cells at 1 m and five at 2 m, where the point at 2.0e6 is still inside the key range; the 1 m
    level has room for two of them, the 2 m level for all"""
    hb, _ = NR.hand_built_cells()
    res = (2.0, 1.0)
    cells = [len(NR.group(hb, r)[0]) for r in res]
    caps = (cells[0] + 5, cells[1] + 2)
    pts = hand_points()
    pyr = make(hb, res, caps)
    levels = OP.build(hb, res, caps)
    want = OP.update(levels, pts, np.eye(4))
    assert raw_update(pyr, pts, 8, 8, np.eye(4)) == want
    assert want[1] == [caps[1], 2, 2, 4] and want[0] == [caps[0], 5, 0, 7]
    assert_levels_are(pyr, levels)
    want = OP.update(levels, pts, np.eye(4))
    assert raw_update(pyr, pts, 8, 8, np.eye(4)) == want and want[1][1:] == [0, 2, 4] and want[0][1:] == [0, 0, 7]
    assert_levels_are(pyr, levels)
    assert pyr.pyramid_info(1) == (caps[1], caps[1], 4) and pyr.pyramid_info(0)[2] == 0
    # cap = 4 < *n_dev = 8: points 0 .. 3, of which index 2 is NaN
    want = OP.update(levels, pts, np.eye(4), cap=4, n=8)
    assert raw_update(pyr, pts, 8, 4, np.eye(4)) == want and want[0][3] == 3 and want[1][2:] == [1, 2]
    assert_levels_are(pyr, levels)


def test_forgetting_bites_on_one_cell_of_one_level():
    rng = np.random.default_rng(3)
    big = 0.1 + 0.8 * rng.random((40, 3))
    small = np.array([1.0, 0.0, 0.0]) + 0.1 + 0.8 * rng.random((8, 3))
    mp = np.concatenate([big, small])                                          # one cell of 48 at 2 m, cells of 40 and 8 at 1 m
    res, caps = (2.0, 1.0), (4, 4)
    pyr, levels, plain = make(mp, res, caps), OP.build(mp, res, caps), OP.build(mp, res, caps)
    assert [list(m["count"]) for m in levels] == [[48], [40, 8]]
    p = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]])
    assert raw_update(pyr, p, 2, 2, np.eye(4), max_cell_points=45) == OP.update(levels, p, np.eye(4), max_cell_points=45)
    OP.update(plain, p, np.eye(4))
    assert [list(m["count"]) for m in levels] == [[47], [41, 9]]
    assert_levels_are(pyr, levels)
    assert levels[0]["icov"].tobytes() != plain[0]["icov"].tobytes()           # the capped cell forgot
    assert levels[1]["icov"].tobytes() == plain[1]["icov"].tobytes() and levels[1]["S"].tobytes() == plain[1]["S"].tobytes()


def test_bad_rows_are_skipped_at_every_level(map_xyz, scans):
    scan = scans[3][0]
    rows = scan.copy()
    rows[17, 0], rows[400, 2], rows[4000, 1] = np.nan, 3.0e6, -np.inf
    clean = np.delete(scan, [17, 400, 4000], axis=0)                           # the survivors and their order are the same
    a, b = make(map_xyz), make(map_xyz)
    ua = a.integrate(dev(rows), len(rows), T_TRUE).result()
    ub = b.integrate(dev(clean), len(clean), T_TRUE).result()
    ca = a.carve(dev(rows), len(rows), T_TRUE, min_pass=1, miss_frames=1).result()
    cb = b.carve(dev(clean), len(clean), T_TRUE, min_pass=1, miss_frames=1).result()
    assert upd_words(ua) == upd_words(ub) and carve_words(ca) == carve_words(cb) and ua[0].points > 4000
    for l in range(3):
        assert_same_cells(raw_level(a, l), raw_level(b, l), l)
    # rows that are bad after the thinning, through the raw calls, against the restatement
    pts = scans[3][1][:64].copy()
    pts[5, 1], pts[9, 0], pts[33, 2] = np.nan, 3.0e6, np.inf                   # 3.0e6: beyond the key range at 2 m too
    levels = OP.build(map_xyz, RESOLUTIONS, CAPACITIES)
    kept = LR.downsample(clean, len(clean), LEAF)[1]
    assert upd_words(ua) == OP.update(levels, kept, T_TRUE)
    assert carve_words(ca) == OP.carve(levels, kept, T_TRUE, min_pass=1, miss_frames=1)
    want = OP.update(levels, pts, T_TRUE)
    assert raw_update(a, pts, 64, 64, T_TRUE) == want and all(w[3] == 61 for w in want)
    want = OP.carve(levels, pts, T_TRUE)
    assert raw_carve(a, pts, 64, 64, T_TRUE) == want and all(w[0] == 61 for w in want)
    assert_levels_are(a, levels)
    a.ctx.check_errors(stream())


# ---- the carve -----------------------------------------------------------------------------------------------------------
def test_three_frames_of_the_phantom_scene(phantom, scans):
    with_pole, only, lv0 = phantom
    levels = copy.deepcopy(lv0)
    pyr, singles = make(with_pole), make_singles(with_pole)
    assert tuple(pyr.level_cells) == PHANTOM_CELLS
    before = [raw_level(pyr, l) for l in range(3)]
    for frame in (1, 2, 3):
        scan, pts = scans[frame]
        want = OP.carve(levels, pts, T_TRUE)
        got = pyr.carve(dev(scan), len(scan), T_TRUE).result()
        one = [s.carve(dev(scan), len(scan), T_TRUE).result() for s in singles]
        print(f"frame {frame}: info per level (rays, seen through, cleared, cut) {want}")
        assert isinstance(got, tuple) and carve_words(got) == carve_words(one) == want == list(PHANTOM_INFO[frame])
        assert all(c.n_points == len(pts) for c in got)
        assert_levels_are_singles(pyr, singles, frame)
        assert_levels_are(pyr, levels, frame)
    for l in range(3):                                                         # no cell that exists without the pole changed
        after = raw_level(pyr, l)
        keep = np.ones(CAPACITIES[l], dtype=bool)
        keep[only[l]] = False
        assert_same_cells({k: after[k][keep] for k in after}, {k: before[l][k][keep] for k in before[l]}, l)
        assert (after["keys"] == before[l]["keys"]).all()                      # a cleared cell keeps its key and its id
    assert [int((raw_level(pyr, l)["count"][only[l]] == 0).sum()) for l in range(3)] == [1, 2, 14]
    # per-level end margins and one margin for all levels
    for em in ((3.0, 1.0, 0.25), 0.5):
        scan, pts = scans[4]
        want = OP.carve(levels, pts, T_TRUE, end_margin=em, min_pass=1, miss_frames=1, through_sigma=2.0)
        got = pyr.carve(dev(scan), len(scan), T_TRUE, end_margin=em, min_pass=1, miss_frames=1, through_sigma=2.0).result()
        assert carve_words(got) == want and sum(w[2] for w in want) > 5
        assert_levels_are(pyr, levels, em)
    pyr.ctx.check_errors(stream())


@pytest.fixture(scope="module")
def box():
    """64 000 points that fill the 8 000 cells of 0.5 m of [-4, 6)^3, eight each: valid Gaussians at all three levels"""
    rng = np.random.default_rng(21)
    c = np.stack(np.meshgrid(*[np.arange(-8, 12)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64) * 0.5
    mp = (c[:, None, :] + 0.05 + 0.4 * rng.random((len(c), 8, 3))).reshape(-1, 3)
    caps = (128, 1024, 8192)
    levels = OP.build(mp, RESOLUTIONS, caps)
    assert [len(m["keys"]) for m in levels] == [125, 1000, 8000] and all(m["valid"].all() for m in levels)
    return mp, caps, levels


def test_tie_rays_scaled_by_every_levels_resolution(box):
    """tie_rays() are made for cells of edge 1; scaled by a power of two every tMax stays exact, and at the level of that
    edge the ray meets the same faces, edges and corners"""
    mp, caps, lv0 = box
    levels = copy.deepcopy(lv0)
    pyr = make(mp, caps=caps)
    kw = dict(min_pass=1, miss_frames=100)
    passes = 0
    for scale in RESOLUTIONS:
        for name, o, q, margin, max_steps, cells, cut in tie_rays():
            p = ((np.asarray(q) - np.asarray(o)) * scale)[None]                # exact: every number is dyadic
            T = pose_at(np.asarray(o) * scale)
            em = [margin * scale] * 3
            want = OP.carve(levels, p, T, end_margin=em, max_steps=max_steps, **kw)
            assert raw_carve(pyr, p, 1, 1, T, end_margin=em, max_steps=max_steps, **kw) == want, (scale, name)
            l = RESOLUTIONS.index(scale)
            assert want[l][0] == 1 and want[l][3] == int(cut) and levels[l]["pass"].sum() <= len(cells), (scale, name)
            passes += int(levels[l]["pass"].sum())
        assert_levels_are(pyr, levels, scale)
    assert passes > 20
    far = pose_at((3.0e6, 0.5, 0.5))                                           # the sensor beyond every level's key range: nothing is cast
    bad = np.array([[1.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]])
    assert raw_carve(pyr, bad, 3, 3, far, **kw) == OP.carve(levels, bad, far, **kw) == [[0, 0, 0, 0]] * 3
    assert_levels_are(pyr, levels, "far sensor")


# ---- the gate and the pose -----------------------------------------------------------------------------------------------
def test_a_closed_gate_changes_no_byte_of_any_level(phantom, scans):
    with_pole, _, _ = phantom
    scan, pts = scans[1]
    pyr = make(with_pole)
    first = pyr.carve(dev(scan), len(scan), T_TRUE).result()                   # state worth keeping
    assert [c.seen_through for c in first] == [2, 2, 14]
    before = [(raw_level(pyr, l), pyr.carve_state(l), pyr.pyramid_info(l)) for l in range(3)]
    assert all(s[0].any() and s[1].any() and s[2].any() for _, s, _ in before)
    # status 2 from an alignment against an empty pyramid: its device status word is the gate
    empty = make(np.zeros((0, 3)))
    pend = empty.submit(dev(scan), len(scan), T_INIT)
    assert pend.result().status == 2
    gate = pend._pose_on_device()[2]
    assert raw_update(pyr, pts, len(pts), len(pts), T_TRUE, gate_ptr=gate) == [[PHANTOM_CELLS[l], 0, 0, 0] for l in range(3)]
    assert raw_carve(pyr, pts, len(pts), len(pts), T_TRUE, gate_ptr=gate, min_pass=1, miss_frames=1) == [[0, 0, 0, 0]] * 3
    # the same through a frame that fails its own alignment
    closed = make(with_pole, min_correspondences=len(pts) + 1)
    r = closed.submit(dev(scan), len(scan), T_INIT, integrate=True, carve=True, carve_options=dict(min_pass=1, miss_frames=1)).result()
    assert r.status == 2 and carve_words(r.map_carve) == [[0, 0, 0, 0]] * 3
    assert upd_words(r.map_update) == [[PHANTOM_CELLS[l], 0, 0, 0] for l in range(3)]
    fresh = make(with_pole)
    for l in range(3):
        cells, state, info = before[l]
        assert_same_cells(raw_level(pyr, l), cells, l)
        assert pyr.pyramid_info(l) == info
        for a, b in zip(pyr.carve_state(l), state):
            assert a.tobytes() == b.tobytes()
        assert_same_cells(raw_level(closed, l), raw_level(fresh, l), l)
        assert not any(a.any() for a in closed.carve_state(l))
    # an open gate (status 0 / 1) lets both through
    opened = torch.tensor([1], dtype=torch.int32, device="cuda")
    assert raw_update(pyr, pts, len(pts), len(pts), T_TRUE, gate_ptr=opened.data_ptr())[0][3] == len(pts)
    assert raw_carve(pyr, pts, len(pts), len(pts), T_TRUE, gate_ptr=opened.data_ptr())[0][0] == len(pts)
    pyr.ctx.check_errors(stream())


def test_a_device_pose_and_a_host_pose_give_the_same_bits(map_xyz, scans):
    pts = scans[2][1]
    T = LR.perturbation(0.3, 5.0, 0.0, 10.0) @ T_TRUE
    a, b = make(map_xyz), make(map_xyz)
    kw = dict(min_pass=1, miss_frames=1)
    assert raw_carve(a, pts, len(pts), len(pts), T, **kw) == raw_carve(b, pts, len(pts), len(pts), T, T_on_device=True, **kw)
    ua, ub = raw_update(a, pts, len(pts), len(pts), T), raw_update(b, pts, len(pts), len(pts), T, T_on_device=True)
    assert ua == ub and all(w[3] == len(pts) and w[1] > 50 for w in ua)
    for l in range(3):
        assert_same_cells(raw_level(a, l), raw_level(b, l), l)
        for x, y in zip(a.carve_state(l), b.carve_state(l)):
            assert x.tobytes() == y.tobytes()


# ---- refusals and rebuilds -----------------------------------------------------------------------------------------------
def test_a_static_pyramid_is_refused(map_xyz, scans):
    from sps_amd import _native
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser
    static = NDTLocaliser(map_xyz, resolutions=RESOLUTIONS, leaf=LEAF)
    scan, pts = scans[1]
    for call in (lambda: static.integrate(dev(scan), len(scan), T_TRUE), lambda: static.carve(dev(scan), len(scan), T_TRUE),
                 lambda: static.submit(dev(scan), len(scan), T_INIT, integrate=True),
                 lambda: static.submit(dev(scan), len(scan), T_INIT, carve=True), lambda: static.pyramid_info(0),
                 lambda: static.carve_state(0), lambda: LocalisationLoop(None, static, T_INIT, update_map=True),
                 lambda: LocalisationLoop(None, static, T_INIT, carve_map=True)):
        with pytest.raises(ValueError):
            call()
    static.level_capacities = CAPACITIES                                       # past the Python checks: the C ABI refuses for itself
    plain = _native.Context(0)
    for loc_ctx in (static.ctx, plain):                                        # a static pyramid, and no pyramid at all
        static.ctx, keep = loc_ctx, static.ctx
        for call in (lambda: raw_update(static, pts[:10], 10, 10, T_TRUE), lambda: raw_carve(static, pts[:10], 10, 10, T_TRUE),
                     lambda: static.ctx.ndt_pyramid_info(0), lambda: static.ctx.ndt_pyramid_carve_cells(0, None, None, None)):
            with pytest.raises(_native.SpsError) as e:
                call()
            assert e.value.code == _native.ERR_INVALID
        static.ctx = keep
    static.level_capacities = None
    static.ctx.check_errors(stream())                                          # the sticky error is unset
    assert static(dev(scan), len(scan), T_INIT).status in (0, 1)
    # bad options reach neither the device nor the map
    dyn = make(map_xyz)
    for bad in (dict(through_sigma=0.0), dict(end_margin=(1.0, -1.0, 1.0)), dict(end_margin=(1.0, 1.0)), dict(min_pass=0),
                dict(miss_frames=0), dict(max_steps=4097)):
        with pytest.raises(ValueError):
            dyn.carve(dev(scan), len(scan), T_TRUE, **bad)
    with pytest.raises(_native.SpsError):
        raw_carve(dyn, pts[:10], 10, 10, T_TRUE, end_margin=(1.0, float("inf"), 1.0))
    with pytest.raises(_native.SpsError):
        raw_update(dyn, pts[:10], 10, 10, T_TRUE, max_cell_points=-1)
    with pytest.raises(ValueError):
        LocalisationLoop(None, dyn, T_INIT, update_map=True, hypotheses=np.eye(4)[None])
    assert _native.lib.sps_version() == 202
    dyn.ctx.check_errors(stream())


def test_one_context_rebuilt_static_dynamic_static(scans):
    from sps_amd import _native
    from sps_amd.datasets.blt_dataset import radius_grid_cells
    rng = np.random.default_rng(11)
    mp = 0.05 + 1.9 * rng.random((300, 3))                                     # the 8 cells of 1 m of [0, 2)^3: one cell of 2 m
    pts = 0.05 + np.array([2.9, 1.9, 1.9]) * rng.random((50, 3))               # those and the 4 cells at 2 <= x < 3
    res, caps = (2.0, 1.0), (4, 16)
    from sps_amd.localiser import NDTLocaliser
    loc = NDTLocaliser(mp, resolutions=res, leaf=LEAF)                         # the first build: static
    xyz = dev(mp)
    keep = [radius_grid_cells(xyz, r) for r in res]
    lv = [(k.contiguous().data_ptr(), s.data_ptr(), p.data_ptr(), len(k), r) for (k, s, p), r in zip(keep, res)]
    assert [v[3] for v in lv] == [1, 8]
    single_before = loc.map_cells()

    def build(dynamic):
        loc.ctx.ndt_pyramid_build(lv, xyz.data_ptr(), len(mp), 6, 0.01, 0.55, stream(), caps if dynamic else None)
        loc.level_capacities = caps if dynamic else None

    def is_static():
        loc.level_capacities = caps
        with pytest.raises(_native.SpsError):
            raw_update(loc, pts, len(pts), len(pts), np.eye(4))
        with pytest.raises(_native.SpsError):
            loc.ctx.ndt_pyramid_info(1)
        loc.level_capacities = None
        for l, r in enumerate(res):
            assert_same_cells(dict(zip(FIELDS, loc.pyramid_cells(l))), NR.cells(mp, r), l)

    is_static()
    build(True)
    levels = OP.build(mp, res, caps)
    assert_levels_are(loc, levels)
    want = OP.update(levels, pts, np.eye(4))
    assert raw_update(loc, pts, len(pts), len(pts), np.eye(4)) == want and want[1][1] == 4 and want[0][1] == 1
    assert_levels_are(loc, levels)
    build(False)
    is_static()
    build(True)                                                                # and a dynamic build starts from the map again
    assert_levels_are(loc, OP.build(mp, res, caps))
    for a, b in zip(loc.map_cells(), single_before):                           # the single map was never touched
        assert a.tobytes() == b.tobytes()
    loc.ctx.check_errors(stream())


# ---- determinism and stream order ----------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes(map_xyz, scans):
    runs = []
    for _ in range(2):
        pyr = make(map_xyz)
        infos = []
        for seed, dy in ((1, 0.0), (2, 6.0), (3, 6.0)):
            s = dev(scans[seed][0])
            T = LR.perturbation(0.0, dy, 0.0, 0.0) @ T_TRUE
            infos.append(carve_words(pyr.carve(s, len(s), T, min_pass=1, miss_frames=2, through_sigma=2.0).result()))
            infos.append(upd_words(pyr.integrate(s, len(s), T, max_cell_points=50).result()))
        runs.append((infos, [raw_level(pyr, l) for l in range(3)], [pyr.carve_state(l) for l in range(3)]))
    assert runs[0][0] == runs[1][0] and any(w[2] > 0 for w in runs[0][0][2])   # cells were cleared on the way
    for l in range(3):
        assert_same_cells(runs[0][1][l], runs[1][1][l], l)
        for a, b in zip(runs[0][2][l], runs[1][2][l]):
            assert a.tobytes() == b.tobytes()


def test_an_alignment_behind_an_update_on_a_side_stream_sees_the_updated_levels(scans):
    sc = changed_scene()
    pyr = make(sc["cut"])
    s1, s2 = dev(scans[1][0]), dev(scans[2][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pa = pyr.submit(s1, len(s1), T_INIT, integrate=True)
        pb = pyr.submit(s2, len(s2), T_INIT)                                   # no synchronisation in between
    a, b = pa.result(), pb.result()
    levels = OP.build(sc["cut"], RESOLUTIONS, CAPACITIES)
    kw = dict(iters=30, level_iters=LEVEL_ITERS)
    plain = OP.align(scans[2][1], levels, T_INIT, **kw)
    assert a.status in (0, 1) and upd_words(a.map_update) == OP.update(levels, scans[1][1], a.pose, gate=a.status)
    assert all(u.founded > 50 for u in a.map_update)
    fwd = OP.align(scans[2][1], levels, T_INIT, **kw)
    rev = OP.align(scans[2][1], levels, T_INIT, reverse=True, **kw)
    spread_t, spread_r = LR.pose_difference(fwd["pose"], rev["pose"])
    tol_t, tol_r = max(100.0 * spread_t, TOL_FLOOR), max(100.0 * spread_r, TOL_FLOOR)
    dt, dr = LR.pose_difference(b.pose, fwd["pose"])
    print(f"spread {spread_t:.3e} m {spread_r:.3e} rad; device vs restatement {dt:.3e} m {dr:.3e} rad; counted {b.n_corr} "
          f"(without the update {plain['n_corr']})")
    assert (b.status, b.iterations) == (fwd["status"], fwd["iterations"])
    np.testing.assert_array_equal(b.levels, fwd["levels"])
    np.testing.assert_array_equal(b.trace[:, 0], fwd["trace"][:, 0])
    assert dt <= tol_t and dr <= tol_r
    assert fwd["trace"][0, 0] > plain["trace"][0, 0]                           # the update shows in the first slot's count
    assert_levels_are(pyr, levels)


# ---- the frame's one buffer ----------------------------------------------------------------------------------------------
def test_the_combined_call_carves_then_updates_and_reports_per_level(phantom, scans):
    """min_pass = 1 and miss_frames = 1: one frame clears, and the update behind it refills what the frame observes"""
    with_pole, _, lv0 = phantom
    scan, pts = scans[1]
    opts = dict(min_pass=1, miss_frames=1, through_sigma=2.0)
    one, parts = make(with_pole), make(with_pole)
    r = one.submit(dev(scan), len(scan), T_INIT, integrate=True, carve=True, carve_options=opts, max_cell_points=60,
                   with_normal=True).result()
    p = parts.submit(dev(scan), len(scan), T_INIT, with_normal=True).result()
    assert r.status in (0, 1) and p.map_carve is None and p.map_update is None
    same_bits(r, p)                                                            # the levels, trace and normal rows keep their places
    c = parts.carve(dev(scan), len(scan), p.pose, **opts).result()
    u = parts.integrate(dev(scan), len(scan), p.pose, max_cell_points=60).result()
    assert isinstance(r.map_carve, tuple) and isinstance(r.map_update, tuple) and len(r.map_carve) == len(r.map_update) == 3
    assert carve_words(r.map_carve) == carve_words(c) and upd_words(r.map_update) == upd_words(u) and all(x.cleared > 0 for x in c)
    assert all(x.n_points == r.n_points for x in r.map_carve + r.map_update)
    for l in range(3):
        assert_same_cells(raw_level(one, l), raw_level(parts, l), l)
        for a, b in zip(one.carve_state(l), parts.carve_state(l)):
            assert a.tobytes() == b.tobytes()
    # and both are the restatement's carve followed by its update, at the pose the device found
    levels = copy.deepcopy(lv0)
    assert OP.carve(levels, pts, r.pose, gate=r.status, **opts) == carve_words(c)
    assert [int((m["count"] == 0).sum()) for m in levels] == [x.cleared for x in c]
    assert OP.update(levels, pts, r.pose, gate=r.status, max_cell_points=60) == upd_words(u)
    assert_levels_are(one, levels)
    # the order is the carve's, then the update's: the cells this frame founds took no hit, as they would the other way round
    swapped = copy.deepcopy(lv0)
    OP.update(swapped, pts, r.pose, max_cell_points=60)
    OP.carve(swapped, pts, r.pose, **opts)
    for l, (m, sw) in enumerate(zip(levels, swapped)):
        n0 = len(lv0[l]["keys"])
        assert u[l].founded > 0 and not one.carve_state(l)[1][n0:].any() and CR.state(sw)[1][n0:].all(), l
    one.ctx.check_errors(stream())


# ---- the loop ------------------------------------------------------------------------------------------------------------
class Recording:
    """the device localiser behind the interface LocalisationLoop uses, keeping every frame's kept rows and guess"""

    def __init__(self, loc):
        self.loc, self.device, self.level_capacities, self.frames = loc, loc.device, loc.level_capacities, []

    def submit_filtered(self, pending, T_init, **kw):
        n = int(pending.count_dev.item())
        self.frames.append((pending._filtered[:n].cpu().numpy(), np.array(T_init, dtype=np.float64), kw))
        return self.loc.submit_filtered(pending, T_init, **kw)


def test_the_closed_loop_follows_the_restatement_on_a_changed_scene(scans):
    """Four frames through LocalisationLoop(update_map=True, carve_map=True) around an online pyramid built from the map with
    a half-space cut away.  The restatement registers every frame on its own levels from the loop's guess (status, slots,
    levels and counts equal, the pose within 100 x the restatement's forward / reversed spread, floor 1e-12) and then carves
    and updates them at the pose the device returned, the one input the two must share for their maps to agree bit for bit."""
    from sps_amd.localiser import LocalisationLoop
    from sps_amd.sps_filters import SPSCVMFilter
    sc = changed_scene()
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(np.ascontiguousarray(sc["cut"], dtype=np.float32))
    like = make(sc["cut"])
    rec = Recording(like)
    f = SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0)     # every point passes
    loop = LocalisationLoop(f, rec, T_INIT, update_map=True, carve_map=True)
    got = [loop.step(scans[k][0]) for k in (1, 2, 3, 4)]
    levels = OP.build(sc["cut"], RESOLUTIONS, CAPACITIES)
    kw = dict(iters=like.iterations, level_iters=like.level_iterations, neighbours=like.neighbours, min_corr=like.min_correspondences,
              outlier_ratio=like.outlier_ratio, tol_t=like.tol_t, tol_r=like.tol_r)
    fwd = OP.align(scans[1][1], levels, T_INIT, **kw)
    rev = OP.align(scans[1][1], levels, T_INIT, reverse=True, **kw)
    spread_t, spread_r = LR.pose_difference(fwd["pose"], rev["pose"])
    tol_t, tol_r = max(100.0 * spread_t, TOL_FLOOR), max(100.0 * spread_r, TOL_FLOOR)
    for i, step in enumerate(got):
        rows, guess, opts = rec.frames[i]
        a = step.pose_result
        assert opts["carve"] and opts["integrate"] and a.status in (0, 1) and not step.flagged, i
        _, pts = LR.downsample(rows, len(rows), like.leaf, like.capacity)
        r = OP.align(pts, levels, guess, **kw)
        dt, dr = LR.pose_difference(a.pose, r["pose"])
        want_c = OP.carve(levels, pts, a.pose, gate=a.status)
        want_u = OP.update(levels, pts, a.pose, gate=a.status)
        print(f"frame {i}: status {a.status}/{r['status']} slots {a.iterations}/{r['iterations']} count {a.n_corr}/{r['n_corr']} "
              f"device vs restatement {dt:.3e} m {dr:.3e} rad (tolerance {tol_t:.3e} m {tol_r:.3e} rad); carve {want_c}; "
              f"update {want_u}")
        assert (a.status, a.iterations, a.n_corr, a.n_points) == (r["status"], r["iterations"], r["n_corr"], len(pts)), i
        np.testing.assert_array_equal(a.levels, r["levels"])
        assert dt <= tol_t and dr <= tol_r, i
        assert carve_words(a.map_carve) == want_c and upd_words(a.map_update) == want_u, i
    assert all(got[0].pose_result.map_update[l].founded > 50 for l in range(3))      # the loop learned the cut half
    assert_levels_are(like, levels)
    like.ctx.check_errors(stream())


# ---- the single map is a pyramid of one level: the two slots of a context -------------------------------------------------
def test_the_single_map_scratch_is_the_scratch_of_a_pyramid_of_one_level():
    from sps_amd import _native
    lib = _native.lib
    for cap in (0, 1, 255, 256, 257, 65536):                                   # SPS_NDT_UPDATE_MAX_POINTS
        assert lib.sps_ndt_map_update_scratch(cap) == lib.sps_ndt_pyramid_update_scratch(cap, 1) > 0, cap
        assert lib.sps_ndt_map_carve_scratch(cap) == lib.sps_ndt_pyramid_carve_scratch(cap, 1) == 0, cap


class TwoSlots:
    """One context with the single dynamic map and a one-level dynamic pyramid of the same resolution and capacity: the 8
    cells of 1 m of [0, 2)^3 and room for 10, so that points which reach the 4 cells at 2 <= x < 3 found 2 and drop 2."""
    RES, CAP = 1.0, 10

    def __init__(self):
        from sps_amd.datasets.blt_dataset import radius_grid_cells
        from sps_amd.localiser import NDTLocaliser
        rng = np.random.default_rng(11)
        self.mp = 0.05 + 1.9 * rng.random((300, 3))
        self.pts = 0.05 + np.array([2.9, 1.9, 1.9]) * rng.random((257, 3))
        self.loc = NDTLocaliser(self.mp, resolution=self.RES, leaf=LEAF, cell_capacity=self.CAP)
        self.ctx, self.resolution, self.resolutions = self.loc.ctx, self.RES, (self.RES,)    # what the raw_* helpers read
        self.xyz = dev(self.mp)
        keys, start, idx = radius_grid_cells(self.xyz, self.RES)
        self.keep = (keys.contiguous(), start, idx)
        assert len(keys) == 8
        self.build_pyramid()

    def map_args(self):
        k, s, p = self.keep
        return (k.data_ptr(), s.data_ptr(), p.data_ptr(), self.xyz.data_ptr(), len(k), len(self.mp), self.RES,
                self.loc.min_points_per_cell, self.loc.eig_ratio)

    def build_pyramid(self):
        k, s, p = self.keep
        self.ctx.ndt_pyramid_build([(k.data_ptr(), s.data_ptr(), p.data_ptr(), len(k), self.RES)], self.xyz.data_ptr(), len(self.mp),
                                   self.loc.min_points_per_cell, self.loc.eig_ratio, self.loc.outlier_ratio, stream(), [self.CAP])

    def snapshot(self, level):
        """every byte the getters of a slot return: the single map (level None) or that level of the pyramid"""
        lv = () if level is None else (level,)
        cells, info, carve_cells = ((self.ctx.ndt_map_cells, self.ctx.ndt_map_info, self.ctx.ndt_map_carve_cells) if level is None else
                                    (self.ctx.ndt_pyramid_cells, self.ctx.ndt_pyramid_info, self.ctx.ndt_pyramid_carve_cells))
        C = self.CAP
        out = [torch.full((C,), -3, dtype=torch.int64, device="cuda"), torch.full((C,), -3, dtype=torch.int32, device="cuda"),
               torch.full((C, 3), -3.0, dtype=torch.float64, device="cuda"), torch.full((C, 6), -3.0, dtype=torch.float64, device="cuda"),
               torch.full((C,), -3, dtype=torch.int32, device="cuda")]
        counters = torch.full((3, C), -3, dtype=torch.int32, device="cuda")
        cells(*lv, *[t.data_ptr() for t in out])
        carve_cells(*lv, counters[0].data_ptr(), counters[1].data_ptr(), counters[2].data_ptr())
        return tuple(t.cpu().numpy().tobytes() for t in out + [counters]) + (info(*lv),)

    def run(self, pyramid, n, gate=None):
        """an update and a carve of the first n points on one slot -> their info words (of the pyramid: level 0's)"""
        from tests.test_hip_ndt_carve import raw_carve as single_carve
        from tests.test_hip_ndt_update import raw_update as single_update
        opts = dict(through_sigma=2.0, min_pass=1, miss_frames=2)
        if not pyramid:
            return (single_update(self, self.pts[:n], n, n, np.eye(4), gate=gate),
                    single_carve(self, self.pts[:n], n, n, np.eye(4), gate=gate, **opts))
        g = None if gate is None else torch.tensor([gate], dtype=torch.int32, device="cuda")
        gp = None if g is None else g.data_ptr()
        return (raw_update(self, self.pts[:n], n, n, np.eye(4), gate_ptr=gp)[0], raw_carve(self, self.pts[:n], n, n, np.eye(4), gate_ptr=gp, **opts)[0])


def test_the_two_slots_of_one_context_do_not_alias():
    """The single map and the pyramid of a context go through one implementation and must not share state: calls on the
    single map leave every byte of the pyramid's getters as built, the same calls on the pyramid then give the same bytes and
    info words, and behind a closed gate neither slot changes."""
    two = TwoSlots()
    fresh = two.snapshot(0)
    assert two.snapshot(None) == fresh and fresh[-1] == (8, 10, 0)
    sizes = (0, 1, 33, 257)                                                    # 257: past the 256-thread block edge
    single = []
    for n in sizes:
        single.append(two.run(False, n))
        assert two.snapshot(0) == fresh, n                                     # the pyramid is as built
    after = two.snapshot(None)
    assert after != fresh and after[-1][0] == 10 and after[-1][2] > 0          # the capacity filled and cells were dropped
    assert [c[0] for _, c in single] == list(sizes)                            # every point cast a ray,
    assert all(0 < u[3] <= n for (u, _), n in zip(single[1:], sizes[1:])) and single[3][0][2] > 0   # some lay in dropped cells
    for n, want in zip(sizes, single):
        assert two.run(True, n) == want, n
        assert two.snapshot(None) == after, n                                  # and the single map is where its own calls left it
    assert two.snapshot(0) == after
    for pyramid in (False, True):                                              # a closed gate: no byte of either slot changes
        u, c = two.run(pyramid, 257, gate=2)
        assert u == [10, 0, 0, 0] and c == [0, 0, 0, 0]
        assert two.snapshot(None) == after and two.snapshot(0) == after
    two.ctx.check_errors(stream())


def test_rebuilding_the_single_map_leaves_the_pyramid_alone():
    from sps_amd import _native
    two = TwoSlots()
    fresh = two.snapshot(None)
    two.run(True, 257)
    pyr = two.snapshot(0)
    assert pyr != fresh and two.snapshot(None) == fresh
    two.ctx.ndt_map_build(*two.map_args(), stream())                           # static: the single map's online getters refuse
    with pytest.raises(_native.SpsError):
        two.ctx.ndt_map_info()
    assert_same_cells(raw_cells(two.loc, 8), NR.cells(two.mp, two.RES))
    assert two.snapshot(0) == pyr
    two.ctx.ndt_map_build_dynamic(*two.map_args(), two.CAP, stream())
    assert two.snapshot(None) == fresh and two.snapshot(0) == pyr
    two.build_pyramid()                                                        # and the other way round
    assert two.snapshot(0) == fresh and two.snapshot(None) == fresh
    two.ctx.check_errors(stream())
