"""GPU tests of distribution-to-distribution NDT registered coarse to fine (sps_ndt_pyramid_source_build,
sps_ndt_pyramid_align_d2d, NDTLocaliser(source="cells", resolutions=..., source_resolutions=...); C ABI: the "NDT localiser,
distribution to distribution, pyramid" section of include/sps_hip.h).  Device against device is bit-equal,
with no tolerance: every level's sources against sps_ndt_source_build, one level against sps_ndt_align_d2d, several levels
against single source="cells" localisers chained from the host.  The numpy restatement
(tests/ndt_d2d_pyramid_reference.py) is compared within the project's rule.  The scene is tests/test_ndt_cpu.py's: 400 x 32
rays, the synthetic map, scan 1 thinned at leaf 0.4 to 4 157 points; map and sources at 2 / 1 / 0.5 m, min_corr = 20; the
start is 0.5 m off along the corridor."""
import math

import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import boundary_inputs as BI
from tests import localiser_reference as LR
from tests import ndt_d2d_pyramid_reference as DP
from tests import ndt_d2d_reference as DR
from tests.helpers import CFG, net_from_params, straddle_params
from tests.test_hip_ndt_d2d import SENTINEL, dev, few_cells, raw_align, raw_build, stream
from tests.test_ndt_cpu import KW, LEAF, T_TRUE, sensor_scan
from tests.test_ndt_d2d_cpu import EIG_RATIO, first_valid

pytestmark = pytest.mark.gpu

RESOLUTIONS = (2.0, 1.0, 0.5)
MIN_CORR = 20
T_START = LR.perturbation(0.5, 0.0, 0.0, 0.0) @ T_TRUE
TOL_FLOOR = 1e-12          # this project's rule for float64 comparisons that differ only in the order of a sum
CELLS = dict(source="cells", leaf=LEAF, min_correspondences=MIN_CORR)


@pytest.fixture(scope="module")
def map_xyz():
    return synthetic.build_map(**KW)[:, :3].astype(np.float64)


@pytest.fixture(scope="module")
def cmaps(map_xyz):
    return DP.pyramid(map_xyz, RESOLUTIONS)


@pytest.fixture(scope="module")
def scene():
    """scan 1, its thinned points and the restatement's source cells of the three levels at min_points 3 and 6 (read-only)"""
    scan = sensor_scan(1)
    pts = LR.downsample(scan, len(scan), LEAF)[1]
    return dict(scan=scan, pts=pts, src={mp: DP.sources(pts, RESOLUTIONS, mp, EIG_RATIO) for mp in (3, 6)})


def make(map_xyz, mp=3, caps=(30, 30, 30), **kw):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(map_xyz, resolutions=RESOLUTIONS, source_resolutions=RESOLUTIONS, source_min_points=mp,
                        iterations=sum(caps), level_iterations=caps, **dict(CELLS, **kw))


@pytest.fixture(scope="module")
def pyr(map_xyz):
    return make(map_xyz)


@pytest.fixture(scope="module")
def singles(map_xyz):
    """one single-map source="cells" localiser per resolution and source_min_points: the sources at the map's resolution"""
    from sps_amd.localiser import NDTLocaliser
    return {mp: [NDTLocaliser(map_xyz, resolution=r, source_min_points=mp, **CELLS) for r in RESOLUTIONS] for mp in (3, 6)}


def status_words(loc, scan, T, **kw):
    """the result and the four status words of a call: (code, slots, sources counted, level)"""
    pend = loc.submit(scan, len(scan), T, **kw)
    res = pend.result()
    o = pend._layout()
    return res, [int(v) for v in pend._host.numpy()[o["status"]:o["n_points"]].view(np.int32)]


def chain(locs, scan, T, caps):
    """the single localisers one after another, each from the end pose of the one before"""
    out = []
    for one, cap in zip(locs, caps):
        r = one(scan, len(scan), T, with_normal=True, iterations=cap)
        assert r.status in (0, 1)                                          # the input's condition: no level fails
        out.append(r)
        T = r.pose
    return out


def assert_is_chain(got, words, rows, levels):
    assert got.pose.tobytes() == rows[-1].pose.tobytes()
    assert got.trace.tobytes() == np.concatenate([r.trace for r in rows]).tobytes()
    assert got.normal.tobytes() == np.concatenate([r.normal for r in rows]).tobytes()
    assert list(got.levels) == sum(([l] * r.iterations for l, r in zip(levels, rows)), [])
    assert words[1:] == [sum(r.iterations for r in rows), rows[-1].n_corr, levels[-1]]
    assert got.n_sources == rows[-1].n_sources and got.n_points == rows[-1].n_points


def same_bits(a, b):
    assert (a.status, a.iterations, a.n_corr, a.n_points, a.n_sources) == (b.status, b.iterations, b.n_corr, b.n_points, b.n_sources)
    for x, y in ((a.pose, b.pose), (a.trace, b.trace), (a.normal, b.normal), (a.levels, b.levels)):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()


# ---- 1. the source build -------------------------------------------------------------------------------------------------
def raw_build_levels(loc, pts, resolutions, min_points, n=None, cap=None, eig_ratio=EIG_RATIO, scratch=None, counts=True):
    """sps_ndt_pyramid_source_build itself on float64 points: (records [L, cap, 10], counts [L, cap], n_src [L, 2]), the rows
    pre-filled"""
    from sps_amd import _native
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    cap = len(pts) if cap is None else cap
    L = len(resolutions)
    buf = np.zeros((max(cap, len(pts), 1), 3))
    buf[:len(pts)] = pts
    p = dev(buf)
    n_dev = torch.tensor([len(pts) if n is None else n], dtype=torch.int32, device="cuda")
    src = torch.full((L, max(cap, 1), 10), SENTINEL, dtype=torch.float64, device="cuda")
    cnt = torch.full((L, max(cap, 1)), -7, dtype=torch.int32, device="cuda")
    n_src = torch.full((L, 2), -7, dtype=torch.int32, device="cuda")
    if scratch is None:
        scratch = torch.empty(_native.lib.sps_ndt_pyramid_source_scratch(cap, L), dtype=torch.uint8, device="cuda")
    loc.ctx.ndt_pyramid_source_build(p.data_ptr(), n_dev.data_ptr(), cap, resolutions, min_points, eig_ratio,
                                     src.data_ptr() if cap else None, cnt.data_ptr() if counts else None, n_src.data_ptr(),
                                     scratch.data_ptr(), stream())
    out = src.cpu().numpy(), cnt.cpu().numpy(), n_src.cpu().numpy()
    loc.ctx.check_errors(stream())
    return out


def assert_levels_are_single_builds(loc, pts, resolutions, min_points, n=None, cap=None, what=""):
    """every level is, byte for byte, what sps_ndt_source_build writes: records, counts, (cells, valid cells) and the rows
    past the cells, which stay as they were"""
    rec, cnt, n_src = raw_build_levels(loc, pts, resolutions, min_points, n, cap)
    for l, (r, m) in enumerate(zip(resolutions, min_points)):
        one = raw_build(loc, pts, n=n, cap=cap, res=r, min_points=m)
        assert rec[l].tobytes() == one[0].tobytes() and cnt[l].tobytes() == one[1].tobytes(), (what, l)
        assert tuple(int(v) for v in n_src[l]) == one[2], (what, l)
    return rec, cnt, n_src


LEVELS = {1: ((1.0,), (6,)), 3: ((2.0, 1.0, 0.5), (6, 3, 2)), 4: ((3.0, 2.0, 1.0, 0.5), (6, 3, 2, 1))}


@pytest.mark.parametrize("L", [1, 3, 4])
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 255, 256, 257, 300])
def test_every_level_is_the_single_source_build(pyr, n, L):
    """300: the capacity, with 340 points offered"""
    pts = few_cells(340 if n == 300 else n)
    res, mps = LEVELS[L]
    _, _, n_src = assert_levels_are_single_builds(pyr, pts, res, mps, cap=300 if n == 300 else max(n, 4))
    if n >= 255:
        assert (n_src[:, 1] > 0).all() and (np.diff(n_src[:, 0]) > 0).all()   # finer levels, more cells


def test_source_build_edges(pyr, scene):
    pts = few_cells(300)
    # equal resolutions on two levels, min_points apart
    rec, _, n_src = assert_levels_are_single_builds(pyr, pts, (1.0, 1.0, 0.5), (6, 3, 3), what="equal resolutions")
    assert n_src[0, 0] == n_src[1, 0] and n_src[0, 1] < n_src[1, 1]
    assert rec[0][:, :9].tobytes() == rec[1][:, :9].tobytes()              # the same cells; only the flags differ
    # rows that are skipped: NaN, infinity, beyond the key range
    bad = pts.copy()
    bad[3, 0], bad[50, 1], bad[120, 2], bad[121, 0] = np.nan, 1048576.5 * 2.0, -np.inf, -1048576.5 * 2.0
    assert_levels_are_single_builds(pyr, bad, *LEVELS[3], what="bad rows")
    # n_dev beyond the capacity and below zero
    assert_levels_are_single_builds(pyr, pts, *LEVELS[3], n=300, cap=200, what="n_dev > cap")
    assert_levels_are_single_builds(pyr, pts, *LEVELS[3], n=-3, what="n_dev < 0")
    # the scene's thinned points, shuffled: the founder order is the new one at every level
    shuffled = scene["pts"][np.random.default_rng(5).permutation(len(scene["pts"]))]
    rec, cnt, n_src = assert_levels_are_single_builds(pyr, shuffled, RESOLUTIONS, (3, 3, 3), what="shuffled")
    want = DP.sources(shuffled, RESOLUTIONS, 3, EIG_RATIO)
    for l, w in enumerate(want):
        assert tuple(n_src[l]) == w["n_src"] and rec[l][:w["n_src"][0]].tobytes() == DR.records(w).tobytes()
    # src_count_dev may be NULL
    a = raw_build_levels(pyr, pts, *LEVELS[3], counts=False)
    assert (a[1] == -7).all() and a[0].tobytes() == raw_build_levels(pyr, pts, *LEVELS[3])[0].tobytes()


def test_two_source_builds_on_one_scratch_give_the_same_bytes(pyr, scene):
    from sps_amd import _native
    pts = scene["pts"]
    scratch = torch.empty(_native.lib.sps_ndt_pyramid_source_scratch(len(pts), 3), dtype=torch.uint8, device="cuda")
    a = raw_build_levels(pyr, pts, RESOLUTIONS, (3, 3, 3), scratch=scratch)
    other = raw_build_levels(pyr, few_cells(257), (0.5, 1.0, 3.0), (1, 2, 3), cap=len(pts), scratch=scratch)   # dirties it
    b = raw_build_levels(pyr, pts, RESOLUTIONS, (3, 3, 3), scratch=scratch)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and other[2][0, 0] != a[2][0, 0]
    assert [tuple(v) for v in a[2]] == [s["n_src"] for s in scene["src"][3]]


def lattice(n):
    """n points of which three in four sit six to a 0.5 m cell, on corners 0.2 m apart inside it, and every fourth alone in a
    2 m cell of its own: cells of several points and of one at every resolution of RESOLUTIONS"""
    i = np.arange(n)
    g, c = i // 8, i % 8
    dense = np.stack([0.5 * g + 0.1 + 0.2 * (c & 1), 0.1 + 0.2 * ((c >> 1) & 1), 0.1 + 0.2 * ((c >> 2) & 1)], axis=1)
    lone = np.stack([-3.0 - 2.0 * i, np.full(n, 0.3), np.full(n, 0.3)], axis=1)
    return np.where((i % 4 == 3)[:, None], lone, dense).reshape(-1, 3)


@pytest.mark.parametrize("n", [0, 1, 33, 257])
def test_the_single_build_and_the_pyramid_of_sources_share_a_scratch(pyr, n):
    """The single source build and the pyramid of sources cut their arrays from one layout function: on one scratch, sized
    for three levels and filled with 0xA5, a single build, a three-level build and the single build again.  The strides of the two layouts differ and no byte
    left by one may reach the other: the single build's bytes are the same before and after, and every level is the single
    build at that level's resolution and min_points on a scratch of its own.  cap 257: one and two workgroups of 256 points,
    one and two of the 32-element rows."""
    from sps_amd import _native
    cap, pts, (res, mps) = 257, lattice(n), LEVELS[3]
    scratch = torch.full((_native.lib.sps_ndt_pyramid_source_scratch(cap, 3),), 0xA5, dtype=torch.uint8, device="cuda")
    before = raw_build(pyr, pts, cap=cap, res=1.0, min_points=3, scratch=scratch)
    rec, cnt, n_src = raw_build_levels(pyr, pts, res, mps, cap=cap, scratch=scratch)
    after = raw_build(pyr, pts, cap=cap, res=1.0, min_points=3, scratch=scratch)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and before[2] == after[2]
    for l, (r, m) in enumerate(zip(res, mps)):
        one = raw_build(pyr, pts, cap=cap, res=r, min_points=m)
        assert rec[l].tobytes() == one[0].tobytes() and cnt[l].tobytes() == one[1].tobytes(), l
        assert tuple(int(v) for v in n_src[l]) == one[2], l
    if n >= 33:                                                         # cells of several points and cells of one, some valid
        c = before[1][:before[2][0]]
        assert (c == 1).any() and (c > 1).any() and 0 < before[2][1] < before[2][0]


def test_source_cells_shows_every_level(pyr, singles, scene):
    scan = dev(scene["scan"])
    for l, one in enumerate(singles[3]):
        a, b = pyr.source_cells(scan, len(scan), level=l), one.source_cells(scan, len(scan))
        for k in ("mean", "cov", "count", "valid"):
            assert a[k].tobytes() == b[k].tobytes(), (l, k)
        assert int(a["valid"].sum()) == scene["src"][3][l]["n_src"][1]
    with pytest.raises(ValueError, match="level must be in"):
        pyr.source_cells(scan, len(scan), level=3)
    with pytest.raises(ValueError, match="level must be in"):
        singles[3][0].source_cells(scan, len(scan), level=1)


def test_source_build_arguments_are_checked(pyr):
    from sps_amd import _native
    p = torch.zeros((8, 3), dtype=torch.float64, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    src = torch.zeros((4, 8, 10), dtype=torch.float64, device="cuda")
    n_src = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    scratch = torch.empty(_native.lib.sps_ndt_pyramid_source_scratch(8, 4), dtype=torch.uint8, device="cuda")
    tail = (src.data_ptr(), None, n_src.data_ptr(), scratch.data_ptr(), stream())
    for res, mps, eig in (((), (), 0.01), ((1.0,) * 5, (1,) * 5, 0.01), ((1.0, 0.0), (1, 1), 0.01), ((1.0, math.inf), (1, 1), 0.01),
                          ((1.0, math.nan), (1, 1), 0.01), ((1.0, 1.0), (1, -1), 0.01), ((1.0,), (1,), 0.0), ((1.0,), (1,), 1.5)):
        with pytest.raises(_native.SpsError):
            pyr.ctx.ndt_pyramid_source_build(p.data_ptr(), n.data_ptr(), 8, res, mps, eig, *tail)
    with pytest.raises(_native.SpsError, match="too many points"):
        pyr.ctx.ndt_pyramid_source_build(p.data_ptr(), n.data_ptr(), 65537, (1.0,), (1,), 0.01, *tail)
    pyr.ctx.check_errors(stream())                                         # never a sticky error


# ---- 2. against single-map localisers ------------------------------------------------------------------------------------
def test_one_level_is_the_single_d2d_call(map_xyz, singles, scene):
    from sps_amd.localiser import NDTLocaliser
    one = NDTLocaliser(map_xyz, resolutions=(1.0,), source_resolutions=(1.0,), source_min_points=6, **CELLS)
    scan = dev(scene["scan"])
    for T, iters in ((T_START, None), (T_START, 3), (T_START, 0)):
        kw = dict(with_normal=True, **({} if iters is None else dict(iterations=iters)))
        a, words = status_words(one, scan, T, **kw)
        b = singles[6][1](scan, len(scan), T, **kw)
        assert words == [b.status, b.iterations, b.n_corr, 0]
        assert a.pose.tobytes() == b.pose.tobytes() and a.trace.tobytes() == b.trace.tobytes()
        assert a.normal.tobytes() == b.normal.tobytes() and a.n_sources == b.n_sources == 246
        assert b.levels is None and len(a.levels) == a.iterations and not a.levels.any()
    assert b.iterations == 0 and a.pose.tobytes() == T_START.tobytes()
    one.ctx.check_errors(stream())


@pytest.mark.parametrize("caps", [(30, 30, 30), (5, 3, 30), (1, 1, 1)])
def test_three_levels_are_three_chained_d2d_calls(map_xyz, singles, scene, caps):
    """budget = the sum of the caps, so no level is cut short by it: the pose and the rows of every slot are those of three
    single source="cells" localisers run one after another with iterations = caps[l]"""
    loc = make(map_xyz, 3, caps)
    scan = dev(scene["scan"])
    got, words = status_words(loc, scan, T_START, with_normal=True)
    rows = chain(singles[3], scan, T_START, caps)
    print(f"caps {caps}: chained status/iterations " + ", ".join(f"{r.status}/{r.iterations}" for r in rows)
          + f"; pyramid status {got.status}, {got.iterations} slots, {got.n_sources} sources")
    assert_is_chain(got, words, rows, (0, 1, 2))
    assert words[0] == rows[-1].status and got.n_sources == 222
    if caps == (5, 3, 30):
        assert [r.status for r in rows[:2]] == [1, 1]                      # both handoffs were forced by the cap
    if caps == (30, 30, 30):
        assert got.status == 0 and LR.pose_difference(got.pose, T_TRUE)[0] < 0.05
    loc.ctx.check_errors(stream())


# ---- 3. the skip rule ----------------------------------------------------------------------------------------------------
def test_a_skipped_finest_level(map_xyz, singles, scene):
    """min_points 6: the finest level has 3 valid sources of 2 872 cells, fewer than min_corr, and is never entered: level 1
    is the last, its convergence is status 0, and n_sources is level 1's"""
    loc = make(map_xyz, 6)
    scan = dev(scene["scan"])
    got, words = status_words(loc, scan, T_START, with_normal=True)
    rows = chain(singles[6][:2], scan, T_START, (30, 30))
    assert_is_chain(got, words, rows, (0, 1))
    assert words[0] == 0 and rows[1].status == 0 and got.n_sources == 246
    assert loc.source_cells(scan, len(scan), level=2)["valid"].sum() == 3


def test_a_skipped_middle_level_and_nothing_beyond_level_0(map_xyz, singles, scene):
    scan = dev(scene["scan"])
    loc = make(map_xyz, (3, 1000, 3))                                      # no cell of the scan has 1000 points
    got, words = status_words(loc, scan, T_START, with_normal=True)
    rows = chain([singles[3][0], singles[3][2]], scan, T_START, (30, 30))
    assert_is_chain(got, words, rows, (0, 2))
    assert words[0] == rows[-1].status == 0
    # nothing qualifies beyond level 0: the coarsest level acts as last; its convergence is status 0, its cap status 1
    loc = make(map_xyz, (3, 1000, 1000))
    got, words = status_words(loc, scan, T_START, with_normal=True)
    one = singles[3][0](scan, len(scan), T_START, with_normal=True)
    assert one.status == 0 and words[0] == 0
    assert_is_chain(got, words, [one], (0,))
    got, words = status_words(loc, scan, T_START, with_normal=True, iterations=3)
    assert words[:2] == [1, 3] and got.trace.tobytes() == one.trace[:3].tobytes()
    loc = make(map_xyz, (3, 1000, 1000), caps=(3, 30, 30))
    got, words = status_words(loc, scan, T_START, with_normal=True)
    assert words == [1, 3, one.trace[2, 0], 0] and got.trace.tobytes() == one.trace[:3].tobytes()


def test_a_level_that_converges_in_the_last_slot_of_the_budget_is_status_1(pyr, singles, scene):
    scan = dev(scene["scan"])
    first = singles[3][0](scan, len(scan), T_START)
    k = first.iterations
    assert first.status == 0 and 1 < k < 30                                # level 0 converges in slot k - 1
    res, words = status_words(pyr, scan, T_START, iterations=k)
    assert words[:2] == [1, k] and words[3] == 0 and not res.levels.any()  # exhausted; the finer levels were not entered
    assert res.trace[-1, 2] < pyr.tol_t and res.trace[-1, 3] < pyr.tol_r   # although its last step was a converged one
    assert res.pose.tobytes() == first.pose.tobytes() and res.n_sources == 335
    nxt = pyr(scan, len(scan), T_START, iterations=k + 1)
    assert list(nxt.levels) == [0] * k + [1] and nxt.status == 1 and nxt.n_sources == 597


# ---- 4. through the C ABI: status 2 and 3, counts around a workgroup ------------------------------------------------------
def raw_pyr_align(loc, recs, n_src, cap, T=T_START, iters=30, caps=None, neighbours=7, min_corr=MIN_CORR):
    """sps_ndt_pyramid_align_d2d itself on hand-uploaded records [L][cap][10] and n_src [L][2]"""
    from sps_amd import _native
    L = len(recs)
    r = torch.zeros((L, max(cap, 1), 10), dtype=torch.float64, device="cuda")
    for l, rec in enumerate(recs):
        rec = np.asarray(rec, dtype=np.float64).reshape(-1, 10)[:cap]
        r[l, :len(rec)] = dev(rec)
    n = torch.tensor(np.asarray(n_src, dtype=np.int32).reshape(L, 2), device="cuda")
    K = max(iters, 1)
    out = torch.zeros(16 + 2 + 32 * K + (K + 1) // 2, dtype=torch.float64, device="cuda")
    scratch = torch.empty(_native.lib.sps_ndt_pyramid_align_d2d_scratch(cap), dtype=torch.uint8, device="cuda")
    base = out.data_ptr()
    caps = (K,) * L if caps is None else caps
    loc.ctx.ndt_pyramid_align_d2d(r.data_ptr(), n.data_ptr(), cap, T, iters, caps, neighbours, min_corr, 1e-4, 1e-5, base,
                                  base + 16 * 8, base + 18 * 8 if iters else None, base + (18 + 4 * iters) * 8 if iters else None,
                                  base + (18 + 32 * K) * 8 if iters else None, scratch.data_ptr(), stream())
    h = out.cpu().numpy()
    loc.ctx.check_errors(stream())
    words = [int(x) for x in h[16:18].view(np.int32)]
    it = words[1]
    return dict(pose=h[:16].reshape(4, 4).copy(), words=words, trace=h[18:18 + 4 * iters].reshape(iters, 4)[:it],
                normal=h[18 + 4 * iters:18 + 32 * iters].reshape(iters, 28)[:it],
                levels=h[18 + 32 * K:].view(np.int32)[:iters].copy())


def raw_chain(locs, recs, n_cells, caps, T=T_START, min_corr=MIN_CORR):
    """sps_ndt_align_d2d on each level's records against that level's single map, chained"""
    out = []
    for loc, rec, n, cap in zip(locs, recs, n_cells, caps):
        r = raw_align(loc, rec, n_src=n, cap=len(rec), T=T, iters=cap, min_corr=min_corr)
        out.append(r)
        T = r["pose"]
    return out


@pytest.mark.parametrize("k", [31, 32, 33])
@pytest.mark.parametrize("over", [False, True])
def test_source_counts_around_a_workgroup(pyr, singles, scene, k, over):
    """hand-made records: every level has exactly k valid sources, k straddling the 32 sources of a workgroup of launch A.
    ``over``: both words of n_src exceed cap_src and are clipped to it."""
    subs = [first_valid(s, k) for s in scene["src"][3]]
    recs = [DR.records(s) for s in subs]
    cap = max(len(r) for r in recs)
    assert all(s["n_src"][1] == k for s in subs)
    n_src = [(len(r) + (1000 if over and len(r) == cap else 0), k + (1000 if over else 0)) for r in recs]
    got = raw_pyr_align(pyr, recs, n_src, cap, iters=9, caps=(3, 3, 3))
    rows = raw_chain(singles[3], recs, [len(r) for r in recs], (3, 3, 3))
    assert [r["status"] for r in rows[:2]] == [1, 1] and all(0 < r["n_corr"] <= k for r in rows)
    assert got["pose"].tobytes() == rows[-1]["pose"].tobytes()
    assert got["trace"].tobytes() == np.concatenate([r["trace"] for r in rows]).tobytes()
    assert got["normal"].tobytes() == np.concatenate([r["normal"] for r in rows]).tobytes()
    assert list(got["levels"]) == [0] * 3 + [1] * 3 + [2] * 3
    assert got["words"] == [rows[-1]["status"], 9, rows[-1]["n_corr"], 2]
    # one source fewer than min_corr on the finer levels: they are skipped, whatever n_src[l][0] says
    got = raw_pyr_align(pyr, recs, n_src, cap, iters=9, caps=(3, 3, 3), min_corr=k + 1 if not over else cap + 1)
    assert got["words"][0] == 2 and got["words"][1] == 1 and got["pose"].tobytes() == T_START.tobytes()


def test_status_2_at_level_0_and_at_a_fine_level_without_cells(map_xyz, pyr, scene):
    recs = [DR.records(s) for s in scene["src"][3]]
    n_src = [s["n_src"] for s in scene["src"][3]]
    cap = max(len(r) for r in recs)
    # level 0 has 335 valid sources: with min_corr = 336 it is too sparse, and level 0 is always entered
    got = raw_pyr_align(pyr, recs, n_src, cap, min_corr=336)
    assert got["words"][:2] == [2, 1] and got["words"][3] == 0 and got["words"][2] < 336
    assert got["pose"].tobytes() == T_START.tobytes() and list(got["levels"][:2]) == [0, -1]
    # a finest level whose map has no cells (a second build replaces the pyramid): entered, since its sources qualify, and
    # final with status 2: the first start pose comes back
    from sps_amd.datasets.blt_dataset import radius_grid_cells
    loc = make(map_xyz)
    scan = dev(scene["scan"])
    before = loc(scan, len(scan), T_START)
    assert before.status == 0 and before.levels[-1] == 2
    xyz = dev(map_xyz)
    groups = [tuple(t.contiguous() for t in radius_grid_cells(xyz, r)) for r in RESOLUTIONS]
    levels = [(k.data_ptr(), s.data_ptr(), p.data_ptr(), 0 if l == 2 else len(k), r)
              for l, ((k, s, p), r) in enumerate(zip(groups, RESOLUTIONS))]
    loc.ctx.ndt_pyramid_build(levels, xyz.data_ptr(), len(xyz), loc.min_points_per_cell, loc.eig_ratio, loc.outlier_ratio, stream())
    res, words = status_words(loc, scan, T_START)
    k = int((before.levels < 2).sum())
    assert words == [2, k + 1, 0, 2] and list(res.levels) == list(before.levels[:k]) + [2]
    assert res.pose.tobytes() == T_START.tobytes() and res.n_sources == 222
    assert res.trace[:k].tobytes() == before.trace[:k].tobytes()
    loc.ctx.check_errors(stream())


def test_status_3_from_degenerate_sources():
    """Sources whose means lie on the x axis, at the identity pose: the first column of J is zero, H[0][0] is exactly 0 and
    the first pivot fails.  At level 0; and at level 1 behind a level 0 whose sources sit on the means of their map cells
    (own cell only): every residual is exactly zero, so is the step, the pose stays the identity and level 0 hands over
    as converged.  Final at either level, and the start pose comes back bit for bit."""
    from sps_amd.localiser import NDTLocaliser
    cells = [(x, y, z) for x in range(-4, 4) for y in range(-2, 2) for z in range(-2, 2)]
    mp = BI.cell_points(cells)
    kw = dict(min_points_per_cell=6, leaf=LEAF, source="cells", min_correspondences=1)
    loc = NDTLocaliser(mp, resolutions=(2.0, 1.0), source_resolutions=(2.0, 1.0), **kw)
    coarse = NDTLocaliser(mp, resolution=2.0, **kw)
    cov = [0.01, 0.0, 0.0, 0.01, 0.0, 0.01]
    axis = np.array([[x + 0.5, 0.0, 0.0] + cov + [1.0] for x in range(-4, 4)])
    _, _, means, _, valid = loc.pyramid_cells(0)
    assert len(means) == 16 and valid.all()
    centred = np.array([list(m) + cov + [1.0] for m in means])
    T = np.eye(4)
    single = raw_align(coarse, axis, T=T, iters=3, min_corr=1)
    assert (single["status"], single["iterations"], single["n_corr"]) == (3, 1, 8)
    got = raw_pyr_align(loc, [axis, centred], [(8, 8), (16, 16)], 16, T=T, iters=4, min_corr=1)
    assert got["words"] == [3, 1, 8, 0] and got["pose"].tobytes() == T.tobytes()
    assert got["trace"].tobytes() == single["trace"].tobytes() and got["normal"].tobytes() == single["normal"].tobytes()
    got = raw_pyr_align(loc, [centred, axis], [(16, 16), (8, 8)], 16, T=T, iters=4, neighbours=1, min_corr=1)
    print("level 0 on its cells' means:", got["trace"][0], "then level 1:", got["words"])
    assert got["trace"][0, 0] == 16 and (got["trace"][0, 2:] == 0).all()   # a zero step: converged, handed over
    assert got["words"] == [3, 2, 8, 1] and list(got["levels"][:3]) == [0, 1, -1] and got["pose"].tobytes() == T.tobytes()
    loc.ctx.check_errors(stream())


def test_align_arguments_are_checked(pyr, scene):
    from sps_amd import _native
    out = torch.zeros(64, dtype=torch.float64, device="cuda")
    args = (out.data_ptr(), out.data_ptr() + 128, out.data_ptr() + 160, None, out.data_ptr() + 320, pyr._d2d_pyr_scratch.data_ptr(),
            stream())
    src, n_src = pyr._src_lv.data_ptr(), pyr._n_src_lv.data_ptr()
    for caps, neighbours in (((30, 30, 0), 7), ((30, 30, 30), 5)):
        with pytest.raises(_native.SpsError):
            pyr.ctx.ndt_pyramid_align_d2d(src, n_src, pyr.capacity, T_START, 2, caps, neighbours, 20, 1e-4, 1e-5, *args)
    plain = _native.Context(0)
    with pytest.raises(_native.SpsError, match="sps_ndt_pyramid_build has not been called"):
        plain.ndt_pyramid_align_d2d(src, n_src, pyr.capacity, T_START, 2, (30,), 7, 20, 1e-4, 1e-5, *args)
    scan = dev(scene["scan"])
    with pytest.raises(ValueError):
        pyr.submit(scan, len(scan), T_START, integrate=True)               # a static pyramid
    for call in (lambda: pyr.submit_batch(scan, len(scan), T_START[None], d2d=True, coarse_to_fine=True),
                 lambda: pyr.relocalise(scan, len(scan), T_START[None], d2d=True, coarse_to_fine=True)):
        with pytest.raises(ValueError, match="d2d=True and coarse_to_fine exclude each other"):
            call()


# ---- 5. against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mp", [3, 6])
def test_full_alignment_matches_the_restatement(map_xyz, cmaps, scene, mp):
    S = scene["src"][mp]
    kw = dict(iters=90, level_iters=(30, 30, 30), min_corr=MIN_CORR)
    fwd, rev = DP.align(S, cmaps, T_START, **kw), DP.align(S, cmaps, T_START, reverse=True, **kw)
    st, sr = LR.pose_difference(fwd["pose"], rev["pose"])
    tol_t, tol_r = max(100.0 * st, TOL_FLOOR), max(100.0 * sr, TOL_FLOOR)
    # exact counts need an input without a source on a cell face and without a weight on the guard's boundary
    assert fwd["faces"] == 0 and fwd["boundary"] == 0 and fwd["status"] == rev["status"] == 0
    res, words = status_words(make(map_xyz, mp), dev(scene["scan"]), T_START)
    dt, dr = LR.pose_difference(res.pose, fwd["pose"])
    print(f"min_points {mp}: spread forward/reversed {st:.3e} m {sr:.3e} rad; device vs restatement {dt:.3e} m {dr:.3e} rad; "
          f"slots per level {np.bincount(res.levels, minlength=3)}, error {LR.pose_difference(res.pose, T_TRUE)[0]:.4f} m")
    assert words == [fwd["status"], fwd["iterations"], fwd["n_corr"], fwd["level"]] and res.n_sources == fwd["n_sources"]
    np.testing.assert_array_equal(res.levels, fwd["levels"])              # so the per-level slot counts
    np.testing.assert_array_equal(res.trace[:, 0], fwd["trace"][:, 0])    # the sources counted in every slot
    assert dt <= tol_t and dr <= tol_r
    assert LR.pose_difference(res.pose, T_TRUE)[0] < 0.05                  # tests/test_ndt_d2d_pyramid_cpu.py's sanity cap


# ---- 6. the map, the stream, the loop ------------------------------------------------------------------------------------
def level_capacities(map_xyz):
    return tuple(2 * len(np.unique(np.floor(map_xyz / r).astype(np.int64), axis=0)) for r in RESOLUTIONS)


def test_an_online_pyramid_registers_as_the_static_one_and_updates_as_the_point_pyramid(map_xyz, pyr, scene):
    """submit(integrate=True, carve=True) on an online pyramid with source cells: the registration has the static pyramid's
    bits, and the map takes the thinned points: every level ends as the point pyramid's level ends when it is carved and
    updated at the same pose"""
    from sps_amd.localiser import NDTLocaliser
    caps = level_capacities(map_xyz)
    online = make(map_xyz, level_capacities=caps)
    points = NDTLocaliser(map_xyz, resolutions=RESOLUTIONS, leaf=LEAF, level_capacities=caps)
    scan = dev(sensor_scan(2))
    same_bits(online(scan, len(scan), T_START, with_normal=True), pyr(scan, len(scan), T_START, with_normal=True))
    got = online(scan, len(scan), T_START, with_normal=True, integrate=True, carve=True)
    same_bits(got, pyr(scan, len(scan), T_START, with_normal=True))
    assert got.status == 0 and len(got.map_update) == len(got.map_carve) == 3
    carved = points.carve(scan, len(scan), got.pose).result()
    updated = points.integrate(scan, len(scan), got.pose).result()
    assert got.map_carve == carved and got.map_update == updated and all(u.points > 0 for u in updated)
    for l in range(3):
        for a, b in zip(online.pyramid_cells(l), points.pyramid_cells(l)):
            assert a.tobytes() == b.tobytes(), l
        assert online.pyramid_info(l) == points.pyramid_info(l)
    online.ctx.check_errors(stream())


def test_submit_filtered_equals_result_then_submit(pyr, map_xyz):
    from sps_amd.sps_filters import SPSFilter
    params = straddle_params(O.random_params(seed=0), synthetic.small_scene(seed=11, n_scan=2500))
    net = net_from_params(params).cuda().eval().freeze()
    f = SPSFilter(net, map_xyz.astype(np.float32), voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=CFG["FILTER"]["THRESHOLD"])
    scan = sensor_scan(4)
    pend = f.submit(scan, T_TRUE)
    pose_pend = pyr.submit_filtered(pend, T_START, with_normal=True)       # queued behind the filter, before the frame's result()
    a = pose_pend.result()
    fres = pend.result()
    assert 0 < len(fres.filtered) <= len(scan)
    b = pyr(fres.filtered.clone(), len(fres.filtered), T_START, with_normal=True)
    assert a.iterations > 3 and a.n_sources > MIN_CORR
    same_bits(a, b)


class RestatementLocaliser:
    """tests/ndt_d2d_pyramid_reference.py behind the interface LocalisationLoop uses"""
    source = "cells"

    def __init__(self, cmaps, like):
        self.cmaps, self.like, self.device, self.resolutions = cmaps, like, like.device, like.resolutions

    def submit_filtered(self, pending, T_init):
        from sps_amd.localiser import PoseResult
        n = int(pending.count_dev.item())
        rows = pending._filtered[:n].cpu().numpy()
        L = self.like
        _, pts = LR.downsample(rows, n, L.leaf, L.capacity)
        S = DP.sources(pts, L.source_resolutions, L.source_level_min_points, L.eig_ratio)
        r = DP.align(S, self.cmaps, T_init, L.iterations, L.level_iterations, L.neighbours, L.min_correspondences,
                     L.outlier_ratio, L.tol_t, L.tol_r)
        res = PoseResult(r["pose"], r["status"], r["iterations"], r["n_corr"], float("nan"), r["trace"], None, len(pts), None,
                         r["levels"], None, r["n_sources"])

        class Done:
            def result(self):
                return res
        return Done()


def test_three_frames_of_the_loop_follow_the_restatement():
    """LocalisationLoop(SPSCVMFilter, the d2d pyramid) over three frames of the synthetic sequence at epsilon = 2 (every
    point passes), against the same loop driven by the restatement: status, slots, levels, counts and sources of every
    frame.  The pose difference is printed only: a frame starts from the poses before it."""
    from sps_amd.localiser import LocalisationLoop
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

    ndt = make(map64)
    got, steps = run(ndt)
    want, ref_steps = run(RestatementLocaliser(DP.pyramid(map64, RESOLUTIONS), ndt))
    for i in range(n):
        a, b = steps[i].pose_result, ref_steps[i].pose_result
        dt, dr = LR.pose_difference(got[i], want[i])
        print(f"frame {i}: status {a.status}/{b.status} slots {a.iterations}/{b.iterations} levels "
              f"{np.bincount(a.levels, minlength=3)}/{np.bincount(b.levels, minlength=3)} count {a.n_corr}/{b.n_corr} sources "
              f"{a.n_sources}/{b.n_sources} device vs restatement {dt:.3e} m {dr:.3e} rad")
        assert (a.status, a.iterations, a.n_corr, a.n_points, a.n_sources) == (b.status, b.iterations, b.n_corr, b.n_points,
                                                                               b.n_sources), i
        np.testing.assert_array_equal(a.levels, b.levels)
        assert not steps[i].flagged
    ndt.ctx.check_errors(stream())


# ---- 7. isolation --------------------------------------------------------------------------------------------------------
def test_the_single_map_and_the_d2d_batch_are_untouched_by_the_pyramid_call(map_xyz, singles, scene):
    """the single map, submit_batch(d2d=True) and score_poses(d2d=True) on the same localiser give the bits they gave before
    the pyramid call, which are those of a localiser without a pyramid"""
    loc = make(map_xyz, 6)
    plain = singles[6][1]
    scan = dev(scene["scan"])
    poses = np.stack([LR.perturbation(o, 0.0, 0.0, 0.0) @ T_TRUE for o in (0.0, 0.2, 0.5)])

    def look(l):
        b = l.submit_batch(scan, len(scan), poses, with_normal=True, iterations=5, d2d=True).result()
        s = l.score_poses(scan, len(scan), poses, d2d=True).result()
        parts = [b.pose, b.scores, b.counts, s[0], s[1]] + [x for r in b.results for x in (r.pose, r.trace, r.normal)]
        return b.best, [r.n_sources for r in b.results], b"".join(np.ascontiguousarray(p).tobytes() for p in parts), \
            b"".join(a.tobytes() for a in l.map_cells())

    before = look(loc)
    res = loc(scan, len(scan), T_START)
    assert res.status == 0 and res.iterations > 3
    assert look(loc) == before == look(plain)
    assert before[1] == [246] * 3
    loc.ctx.check_errors(stream())
