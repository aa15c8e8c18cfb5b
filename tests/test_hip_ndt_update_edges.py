"""GPU tests of the online NDT map's update (sps_ndt_map_update, sps_ndt_pyramid_update) on the hand-built inputs of
tests/ndt_update_edge_inputs.py: cells of more than 64 batch points, cell lists across the 2048-index groups of the ordering
bitmap, the full 65 536-point limit, more touched cells than workgroups, a capacity cut beyond the first 1024 points, thousands
of points on one new key, hash probes that wrap past the end of a table, cell faces, and the forgetting branch at its boundary.
tests/test_ndt_update_edges_cpu.py shows that each input has the property its case rests on.

Every case calls the C entry point itself on float64 points under the identity pose and compares the four info words and then
the whole map (keys, counts, means and inverse covariances as bytes, every row of the capacity, the map's info) with
tests/ndt_update_reference.py.  Nothing on this path has an open sum order, so no tolerance appears anywhere in this file."""
import copy

import numpy as np
import pytest

from tests import ndt_carve_reference as CR
from tests import ndt_online_pyramid_reference as OP
from tests import ndt_reference as NR
from tests import ndt_update_edge_inputs as E
from tests import ndt_update_reference as UR
from tests.test_hip_ndt_carve import assert_state_is, pose_at, raw_carve
from tests.test_hip_ndt_online_pyramid import assert_levels_are, assert_levels_are_singles
from tests.test_hip_ndt_online_pyramid import make as make_pyramid
from tests.test_hip_ndt_online_pyramid import make_singles
from tests.test_hip_ndt_online_pyramid import raw_update as raw_pyramid_update
from tests.test_hip_ndt_update import assert_map_is, assert_same_cells, cells_of, dev, make, raw_cells, raw_update, stream  # noqa: F401
from tests.test_ndt_cpu import LEAF

pytestmark = pytest.mark.gpu

EYE = np.eye(4)
NONE = np.zeros((0, 3))


def step(loc, m, pts, n=None, cap=None, what="", **kw):
    """one sps_ndt_map_update on ``loc`` and one UR.update on ``m``: the info words, then the whole map"""
    cap = len(pts) if cap is None else cap
    n = len(pts) if n is None else n
    want = UR.update(m, pts, EYE, cap=cap, n=n, max_cell_points=kw.get("max_cell_points", 0))
    assert raw_update(loc, pts, n, cap, EYE, **kw) == want, what
    assert_map_is(loc, m, what)
    return want


# ---- the 64-point chunks ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    return [E.dense_cells(seed) for seed in (1, 2, 3)]


def test_dense_cells(dense):
    dyn, m = make(NONE, capacity=16), UR.build(NONE, 16)
    assert step(dyn, m, dense[0], what="found") == [9, 9, 0, 879]
    assert step(dyn, m, dense[1], what="merge") == [9, 0, 0, 879]
    assert step(dyn, m, dense[2], what="forget", max_cell_points=100) == [9, 0, 0, 879]
    assert sorted(m["count"]) == sorted(min(2 * c, 100) + c for c in E.DENSE_COUNTS)
    dyn.ctx.check_errors(stream())


# ---- the ordering bitmap ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bitmap():
    return E.bitmap_groups()


@pytest.mark.parametrize("n", E.BITMAP_COUNTS)
def test_bitmap_groups(bitmap, n):
    dyn, m = make(NONE, capacity=256), UR.build(NONE, 256)
    a = step(dyn, m, bitmap, n=n, cap=E.BITMAP_N, what=n)
    assert a[3] == n and a[1] >= 193 and a[2] == 0
    # once more on the cells that now exist, with the pose on the device
    assert step(dyn, m, bitmap, n=n, cap=E.BITMAP_N, what=n, T_on_device=True) == [a[0], 0, 0, n]
    straddle = int(np.nonzero(m["keys"] == NR.cell_key(np.array(E.BITMAP_SPECIAL_CELLS[0])))[0][0])
    assert m["count"][straddle] == 2 * sum(1 for i in E.BITMAP_STRADDLE if i < n)
    dyn.ctx.check_errors(stream())


def test_full_limit():
    pts = E.full_limit()
    dyn, m = make(NONE, capacity=1024), UR.build(NONE, 1024)
    assert step(dyn, m, pts, what="found") == [513, 513, 0, 65536]
    assert step(dyn, m, pts, what="forget", max_cell_points=100) == [513, 0, 0, 65536]
    dyn.ctx.check_errors(stream())


# ---- the grid-stride loop over the touched cells ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,capacity", [(300, 512), (3, 3)])
def test_many_cells(k, capacity):
    pts = E.many_cells(k)
    dyn, m = make(NONE, capacity=capacity), UR.build(NONE, capacity)
    assert step(dyn, m, pts, what="forward") == [k, k, 0, k]
    assert step(dyn, m, pts[::-1], what="reversed") == [k, 0, 0, k]
    assert step(dyn, m, pts, what="forward again") == [k, 0, 0, k] and (m["count"] == 3).all()
    dyn.ctx.check_errors(stream())


# ---- the founder scan ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def founders():
    return E.founder_run(), E.founder_start_map()


@pytest.mark.parametrize("start", [0, 5])
@pytest.mark.parametrize("cut", E.FOUNDER_CUTS)
def test_founder_cut(founders, cut, start):
    pts, start_map = founders
    mp = start_map if start else NONE
    dyn, m = make(mp, capacity=start + cut), UR.build(mp, start + cut)
    assert len(m["keys"]) == start
    a = step(dyn, m, pts, what="first")
    assert a[:3] == [start + cut, cut, 2500 - cut] and cut < a[3] < 3000
    b = step(dyn, m, pts, what="second")                                       # founded 0, the same keys dropped again
    assert b == [start + cut, 0, 2500 - cut, a[3]] and dyn.map_info() == (start + cut, start + cut, 2 * (2500 - cut))
    dyn.ctx.check_errors(stream())


# ---- one key under contention ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_one_key(which):
    pts, again = E.one_key(5000)[which], E.one_key(5000, seed=51)[which]
    dyn, m = make(NONE, capacity=4), UR.build(NONE, 4)
    assert step(dyn, m, pts, what="found") == [1 + which, 1 + which, 0, 5000]
    assert step(dyn, m, again, what="merge") == [1 + which, 0, 0, 5000]
    assert sorted(m["count"]) == [[10000], [5000, 5000]][which]
    dyn.ctx.check_errors(stream())


# ---- probing that wraps ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cluster():
    return E.hash_cluster_cells(), E.hash_cluster()


def test_hash_cluster_builds(cluster):
    """(a) the static build and the dynamic build from the cluster's points"""
    from sps_amd.localiser import NDTLocaliser
    cells, pts = cluster
    static = NDTLocaliser(pts, resolution=1.0, leaf=LEAF)
    want = NR.cells(pts, 1.0)
    assert len(want["keys"]) == len(cells) == 20 and want["valid"].all()
    assert_same_cells(cells_of(static), want)
    static.ctx.check_errors(stream())
    dyn = make(pts, capacity=32)
    assert_map_is(dyn, UR.build(pts, 32))
    dyn.ctx.check_errors(stream())


@pytest.mark.parametrize("capacity", [32, 4096])
def test_hash_cluster_updates_and_carve(cluster, capacity):
    cells, pts = cluster
    dyn, m = make(NONE, capacity=capacity), UR.build(NONE, capacity)
    assert step(dyn, m, pts, what="(b) found") == [20, 20, 0, 160]             # the update's hash and the map's both wrap
    assert step(dyn, m, pts, what="(c) merge") == [20, 0, 0, 160]              # every lookup probes across the wrap
    assert (m["count"] == 16).all() and m["valid"].all()
    # (d) one ray into the middle of every cluster cell
    o = np.array([0.3, 0.4, 0.2])
    ends = cells.astype(np.float64) + 0.5
    rays = ends - o
    assert (E.cell_index(rays + o) == cells).all()
    want = CR.carve(m, rays, pose_at(o))
    assert raw_carve(dyn, rays, len(rays), len(rays), pose_at(o)) == want and want[0] == 20
    assert (CR.state(m)[1] == 1).all()                                         # a hit of exactly 1 in every cell
    assert_state_is(dyn, m, "(d) carve")
    dyn.ctx.check_errors(stream())


# ---- cell faces ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", E.LATTICE_RES)
def test_lattice(res):
    from sps_amd.localiser import NDTLocaliser
    pts, inner = E.lattice(res)
    built = NDTLocaliser(pts[inner], resolution=res, leaf=LEAF, cell_capacity=1024)
    m = UR.build(pts[inner], 1024, res)
    assert_map_is(built, m, "built")
    n0 = len(m["keys"])
    assert step(built, m, pts, what="built + update") == [n0 + 2, 2, 0, len(pts) - 2]   # the two admitted guard cells
    dyn = NDTLocaliser(NONE, resolution=res, leaf=LEAF, cell_capacity=1024)
    e = UR.build(NONE, 1024, res)
    assert step(dyn, e, pts, what="update") == [n0 + 2, n0 + 2, 0, len(pts) - 2]
    built.ctx.check_errors(stream())
    dyn.ctx.check_errors(stream())


# ---- forgetting ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", E.FORGET_BATCHES)
@pytest.mark.parametrize("max_cell_points", [0, 1, 2, E.FORGET_MAX])
def test_forgetting(max_cell_points, batch):
    stored, batches = E.forgetting()
    dyn, m = make(stored, capacity=4), UR.build(stored, 4)
    plain = copy.deepcopy(m)
    assert step(dyn, m, batches[batch], what="first", max_cell_points=max_cell_points) == [4, 0, 0, 4 * batch]
    UR.update(plain, batches[batch], EYE)
    forgot = [c > max_cell_points >= 2 for c in E.FORGET_STORED]
    assert list(m["count"]) == [(max_cell_points if f else c) + batch for f, c in zip(forgot, E.FORGET_STORED)]
    assert [m["S"][i].tobytes() != plain["S"][i].tobytes() for i in range(4)] == forgot
    step(dyn, m, batches[batch], what="second", max_cell_points=max_cell_points)
    dyn.ctx.check_errors(stream())


# ---- the pyramid path ------------------------------------------------------------------------------------------------------
PYRAMIDS = ((4.0, 2.0, 1.0, 0.5), (2.0, 1.0, 0.5))
# a different small capacity per level (keyed by resolution); the founder run's cut bites at 1 m only
PYRAMID_CAPS = {
    "dense": {4.0: 8, 2.0: 12, 1.0: 16, 0.5: 128},
    "bitmap": {4.0: 64, 2.0: 128, 1.0: 256, 0.5: 2048},
    "founder": {4.0: 256, 2.0: 1024, 1.0: 1025, 0.5: 4096},
    "cluster": {4.0: 24, 2.0: 28, 1.0: 32, 0.5: 256},
}


def pyramid_step(pyr, singles, levels, pts, what="", **kw):
    """one sps_ndt_pyramid_update, the same call on every single online map, and UR.update on every level"""
    want = OP.update(levels, pts, EYE, max_cell_points=kw.get("max_cell_points", 0))
    assert raw_pyramid_update(pyr, pts, len(pts), len(pts), EYE, **kw) == want, what
    assert [raw_update(one, pts, len(pts), len(pts), EYE, **kw) for one in singles] == want, what
    assert_levels_are(pyr, levels, what)
    assert_levels_are_singles(pyr, singles, what)
    return want


def pyramid_of(case, resolutions):
    caps = tuple(PYRAMID_CAPS[case][r] for r in resolutions)
    kw = dict(level_iterations=(10,) * len(resolutions))
    return make_pyramid(NONE, resolutions, caps, **kw), make_singles(NONE, resolutions, caps), OP.build(NONE, resolutions, caps)


@pytest.mark.parametrize("resolutions", PYRAMIDS)
def test_pyramid_dense_cells(dense, resolutions):
    pyr, singles, levels = pyramid_of("dense", resolutions)
    a = pyramid_step(pyr, singles, levels, dense[0], "found")
    assert all(w[2] == 0 and w[3] == 879 for w in a)
    pyramid_step(pyr, singles, levels, dense[1], "merge")
    pyramid_step(pyr, singles, levels, dense[2], "forget", max_cell_points=100)
    assert levels[0]["count"].max() >= 400                                     # the coarse cells hold several hundred points
    pyr.ctx.check_errors(stream())


@pytest.mark.parametrize("resolutions", PYRAMIDS)
def test_pyramid_bitmap_groups(bitmap, resolutions):
    pyr, singles, levels = pyramid_of("bitmap", resolutions)
    a = pyramid_step(pyr, singles, levels, bitmap, "found")
    assert all(w[2] == 0 and w[3] == E.BITMAP_N for w in a)
    pyramid_step(pyr, singles, levels, bitmap, "merge", T_on_device=True)
    pyr.ctx.check_errors(stream())


@pytest.mark.parametrize("resolutions", PYRAMIDS)
def test_pyramid_founder_cut(founders, resolutions):
    pts = founders[0]
    pyr, singles, levels = pyramid_of("founder", resolutions)
    a = pyramid_step(pyr, singles, levels, pts, "first")
    b = pyramid_step(pyr, singles, levels, pts, "second")
    for r, wa, wb in zip(resolutions, a, b):                                   # the cut bites on the 1 m level only
        assert (wa[2] > 0) == (r == 1.0) and wb[1] == 0 and wb[2] == wa[2]
    one = resolutions.index(1.0)
    assert a[one][:3] == [1025, 1025, 1475] and pyr.pyramid_info(one) == (1025, 1025, 2950)
    pyr.ctx.check_errors(stream())


@pytest.mark.parametrize("resolutions", PYRAMIDS)
def test_pyramid_hash_cluster(cluster, resolutions):
    pts = cluster[1]
    pyr, singles, levels = pyramid_of("cluster", resolutions)
    a = pyramid_step(pyr, singles, levels, pts, "(b) found")
    b = pyramid_step(pyr, singles, levels, pts, "(c) merge")
    one = resolutions.index(1.0)
    assert a[one] == [20, 20, 0, 160] and all(w[1] == 0 and w[2] == 0 and w[3] == 160 for w in b)
    pyr.ctx.check_errors(stream())
