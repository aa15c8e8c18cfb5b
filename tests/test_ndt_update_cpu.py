"""CPU tests of the online NDT map's numpy restatement (tests/ndt_update_reference.py) and of the changed scene the GPU
test re-uses.  No GPU."""
import numpy as np
import pytest

from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_reference as NR
from tests import ndt_update_reference as UR
from tests.test_ndt_cpu import KW, LEAF, T_INIT, T_TRUE, sensor_scan

TOL_FLOOR = 1e-12              # this project's rule for float64 comparisons that differ only in the order of a sum
CUT_X = 0.0                    # the changed scene: the map lost everything at x > CUT_X (the sensor sits at x = 0.8)
CAPACITY = 4096


def thinned(seed):
    scan = sensor_scan(seed)
    return LR.downsample(scan, len(scan), LEAF)[1]


@pytest.fixture(scope="module")
def map_xyz():
    return synthetic.build_map(**KW)[:, :3].astype(np.float64)


def changed_scene():
    """The map with the half-space x > CUT_X removed, and thinned scans 1 (integrated) and 2 (aligned) taken at T_TRUE."""
    full = synthetic.build_map(**KW)[:, :3].astype(np.float64)
    return dict(full=full, cut=full[full[:, 0] <= CUT_X], frame=thinned(1), probe=thinned(2))


def by_key(c):
    o = np.argsort(c["keys"], kind="stable")
    return {k: c[k][o] for k in ("keys", "count", "mean", "icov", "valid")}


def frob(m6):
    return np.sqrt((m6 ** 2).sum(axis=1) + (m6[:, [1, 2, 4]] ** 2).sum(axis=1))


# ---- one update ----------------------------------------------------------------------------------------------------------
def test_an_empty_map_plus_one_update_equals_the_static_cells(map_xyz):
    m = UR.build(np.zeros((0, 3)), CAPACITY)
    assert len(m["keys"]) == 0
    info = UR.update(m, map_xyz, np.eye(4))
    want = NR.cells(map_xyz, 1.0)
    assert info == [len(want["keys"]), len(want["keys"]), 0, len(map_xyz)]
    got = by_key(m)
    for k in ("keys", "count", "mean", "icov", "valid"):
        assert got[k].tobytes() == np.asarray(want[k]).tobytes(), k
    assert 1000 < got["valid"].sum() < len(got["valid"])


def test_the_build_equals_the_static_cells(map_xyz):
    m = UR.build(map_xyz, CAPACITY)
    want = NR.cells(map_xyz, 1.0)
    for k in ("keys", "count", "mean", "icov", "valid"):
        assert m[k].tobytes() == np.asarray(want[k]).tobytes(), k


def test_merge_route_against_rebuild_route(map_xyz):
    """Means and inverse covariances of map + one scan: the merged moments against the two-pass rebuild over the union.
    Tolerance: 100 x the spread between each route's own forward and reversed point orders (the larger of the two),
    relative to the Frobenius norm of the inverse covariance (means: to the largest coordinate), floored at 1e-12."""
    frame = thinned(1)

    def both(rev):
        mp = map_xyz[::-1] if rev else map_xyz
        fr = frame[::-1] if rev else frame
        m = UR.build(mp, CAPACITY)
        UR.update(m, fr, T_TRUE)
        return by_key(m), by_key(UR.rebuild(m))
    mf, rf = both(False)
    mr, rr = both(True)
    for x in (mr, rf, rr):
        np.testing.assert_array_equal(x["keys"], mf["keys"])
        np.testing.assert_array_equal(x["count"], mf["count"])
    v = mf["valid"] & rf["valid"] & mr["valid"] & rr["valid"]
    assert v.sum() > 1000
    nrm = frob(rf["icov"][v])
    scale = np.abs(rf["mean"]).max()
    spread = max(float((frob(mf["icov"][v] - mr["icov"][v]) / nrm).max()), float((frob(rf["icov"][v] - rr["icov"][v]) / nrm).max()))
    spread_mean = max(float(np.abs(mf["mean"] - mr["mean"]).max() / scale), float(np.abs(rf["mean"] - rr["mean"]).max() / scale))
    tol, tol_mean = max(100.0 * spread, TOL_FLOOR), max(100.0 * spread_mean, TOL_FLOOR)
    got = float((frob(mf["icov"][v] - rf["icov"][v]) / nrm).max())
    got_mean = float(np.abs(mf["mean"] - rf["mean"]).max() / scale)
    print(f"icov: forward/reversed spread {spread:.3e} -> tolerance {tol:.3e}; merge vs rebuild {got:.3e}")
    print(f"mean: forward/reversed spread {spread_mean:.3e} -> tolerance {tol_mean:.3e}; merge vs rebuild {got_mean:.3e}")
    assert got <= tol and got_mean <= tol_mean
    assert (mf["valid"] != rf["valid"]).sum() == 0


def hand_points():
    """Eight points (identity pose, resolution 1): cells A = (0,0,0), B = (5,0,0), C = (9,0,0), D = (-3,0,0) in the order
    of their founders 0, 1, 3, 6; index 2 is NaN, index 5 beyond the guard."""
    return np.array([[0.5, 0.5, 0.5], [5.5, 0.5, 0.5], [np.nan, 0.0, 0.0], [9.5, 0.5, 0.5], [0.25, 0.5, 0.5],
                     [2.0e6, 0.5, 0.5], [-2.5, 0.5, 0.5], [5.25, 0.25, 0.5]])


def test_founder_order_and_the_capacity_rule():
    key = lambda c: int(NR.cell_key(np.array(c)))
    pts = hand_points()
    m = UR.build(np.zeros((0, 3)), 8, min_points=2)
    assert UR.update(m, pts, np.eye(4)) == [4, 4, 0, 6]                         # the NaN and the far point are not counted
    assert [int(k) for k in m["keys"]] == [key([0, 0, 0]), key([5, 0, 0]), key([9, 0, 0]), key([-3, 0, 0])]
    assert list(m["count"]) == [2, 2, 1, 1] and list(m["valid"]) == [True, True, False, False]
    # capacity 2: founders 0 and 1 get ids, the cells of founders 3 and 6 are dropped with their points
    m = UR.build(np.zeros((0, 3)), 2, min_points=2)
    assert UR.update(m, pts, np.eye(4)) == [2, 2, 2, 4]
    assert [int(k) for k in m["keys"]] == [key([0, 0, 0]), key([5, 0, 0])] and list(m["count"]) == [2, 2]
    assert UR.update(m, pts, np.eye(4)) == [2, 0, 2, 4] and list(m["count"]) == [4, 4] and m["dropped"] == 4
    # the order of the points decides who is dropped, nothing else
    m = UR.build(np.zeros((0, 3)), 2, min_points=2)
    assert UR.update(m, pts[::-1], np.eye(4)) == [2, 2, 2, 3]
    assert [int(k) for k in m["keys"]] == [key([5, 0, 0]), key([-3, 0, 0])]
    # cap and n cut the list from the end
    m = UR.build(np.zeros((0, 3)), 8)
    assert UR.update(m, pts, np.eye(4), cap=4) == [3, 3, 0, 3]
    m = UR.build(np.zeros((0, 3)), 8)
    assert UR.update(m, pts, np.eye(4), n=1) == [1, 1, 0, 1]


def test_forgetting_preserves_the_covariance():
    rng = np.random.default_rng(3)
    pts = 0.1 + 0.8 * rng.random((40, 3))
    m = UR.build(pts, 4)
    cov = m["S"][0] / (m["count"][0] - 1)
    # the cap bites at the next update: S is rescaled before the merge, so merging one point that sits on the mean shows it
    m2 = UR.build(pts, 4)
    UR.update(m2, m["mean"][:1].copy(), np.eye(4), max_cell_points=10)
    assert m2["count"][0] == 11
    # after the cap: n = 10 and S * (9 / 39); the point on the mean has delta = 0 and S_b = 0, so S' is the capped S
    capped = m2["S"][0] / 9.0
    print("relative change of S / (n - 1) under the cap:", float(np.abs(capped - cov).max() / np.abs(cov).max()))
    assert np.abs(capped - cov).max() <= 1e-15 * np.abs(cov).max()
    m3 = UR.build(pts, 4)
    UR.update(m3, m["mean"][:1].copy(), np.eye(4), max_cell_points=40)          # n = 40 is not above the cap
    assert m3["count"][0] == 41 and m3["S"][0].tobytes() != m2["S"][0].tobytes()


def test_a_five_point_cell_plus_one_point_becomes_valid():
    hb, names = NR.hand_built_cells()
    m = UR.build(hb, 16)
    row = int(np.nonzero(m["keys"] == NR.cell_key(names["five"]))[0][0])
    assert m["count"][row] == 5 and not m["valid"][row]
    other = {k: m[k].copy() for k in ("count", "mean", "icov", "valid", "S")}
    p = np.asarray(names["five"], dtype=np.float64)[None] + [[0.5, 0.4, 0.6]]
    assert UR.update(m, p, np.eye(4)) == [len(m["keys"]), 0, 0, 1]
    assert m["count"][row] == 6 and m["valid"][row]
    rb = by_key(UR.rebuild(m))
    r2 = int(np.nonzero(rb["keys"] == NR.cell_key(names["five"]))[0][0])
    np.testing.assert_allclose(m["icov"][row], rb["icov"][r2], rtol=1e-9)
    for k, a in other.items():                                                  # untouched cells keep every bit
        keep = np.arange(len(a)) != row
        assert m[k][keep].tobytes() == a[keep].tobytes(), k


def test_a_closed_gate_changes_nothing(map_xyz):
    m = UR.build(map_xyz[::50], CAPACITY)
    before = {k: np.array(m[k]).copy() for k in ("keys", "count", "mean", "icov", "valid", "S")}
    for gate in (2, 3, -1):
        assert UR.update(m, thinned(1), T_TRUE, gate=gate) == [len(before["keys"]), 0, 0, 0]
        for k, a in before.items():
            assert np.array(m[k]).tobytes() == a.tobytes(), (gate, k)
    for gate in (0, 1):
        assert UR.update(m, thinned(1), T_TRUE, gate=gate)[3] > 0


# ---- the changed scene ---------------------------------------------------------------------------------------------------
def test_a_changed_scene_is_learnt():
    sc = changed_scene()
    full = NR.align(sc["probe"], NR.cells(sc["full"], 1.0), T_INIT)
    m = UR.build(sc["cut"], CAPACITY)
    before = NR.align(sc["probe"], UR.as_cmap(m), T_INIT)
    assert before["status"] == 0 and before["n_corr"] < full["n_corr"]          # the cut shows
    info = UR.update(m, sc["frame"], T_TRUE)
    assert info[1] > 0 and info[2] == 0
    after = NR.align(sc["probe"], UR.as_cmap(m), T_INIT)
    et0, er0 = LR.pose_difference(before["pose"], T_TRUE)
    et1, er1 = LR.pose_difference(after["pose"], T_TRUE)
    print(f"counted: full map {full['n_corr']}, cut map {before['n_corr']}, after one frame {after['n_corr']}; "
          f"error {et0:.3e} m {er0:.3e} rad -> {et1:.3e} m {er1:.3e} rad")
    assert after["status"] == 0 and after["n_corr"] > before["n_corr"]
    assert et1 <= et0 and er1 <= er0
