"""CPU tests of the free-space carving's numpy restatement (tests/ndt_carve_reference.py), of the hand-made rays and of the
phantom scene the GPU test re-uses.  No GPU."""
import numpy as np
import pytest

from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_carve_reference as CR
from tests import ndt_reference as NR
from tests import ndt_update_reference as UR
from tests.test_ndt_cpu import KW, LEAF, T_TRUE, sensor_scan

CAPACITY = 4096
PHANTOM_XY, PHANTOM_R, PHANTOM_Z, PHANTOM_N = (4.3, 1.4), 0.3, (-0.9, 0.9), 1500


def thinned(seed):
    scan = sensor_scan(seed)
    return LR.downsample(scan, len(scan), LEAF)[1]


def phantom_pole():
    """1 500 points of a pole no scan sees: radius 0.3 around (4.3, 1.4), z in [-0.9, 0.9]"""
    rng = np.random.default_rng(0)
    r = PHANTOM_R * np.sqrt(rng.random(PHANTOM_N))
    th = 2.0 * np.pi * rng.random(PHANTOM_N)
    z = PHANTOM_Z[0] + (PHANTOM_Z[1] - PHANTOM_Z[0]) * rng.random(PHANTOM_N)
    return np.c_[PHANTOM_XY[0] + r * np.cos(th), PHANTOM_XY[1] + r * np.sin(th), z]


def phantom_scene():
    """(the map's points with the phantom pole, the ids of the cells that only the phantom fills)"""
    mp = synthetic.build_map(**KW)[:, :3].astype(np.float64)
    with_pole = np.concatenate([mp, phantom_pole()])
    have = set(int(k) for k in NR.group(mp, 1.0)[0])
    keys = NR.group(with_pole, 1.0)[0]
    return with_pole, np.array([i for i, k in enumerate(keys) if int(k) not in have])


def tie_rays():
    """Hand-made rays on cells of edge 1: (name, o, q, end_margin, max_steps, the cells visited in order, cut).  Every
    number is a small multiple of a power of two, so each tMax is exact and the expected lists follow from the rules alone."""
    return [
        # tMax_x = 1/8, 3/8, 5/8, 7/8 and s_end = 3/4: the fourth cell is the last
        ("axis-parallel", (0.5, 0.5, 0.5), (4.5, 0.5, 0.5), 1.0, 512, [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)], False),
        # y = 1.0 lies on a face and never changes: floor puts the whole ray into the cells with y index 1
        ("in a cell face", (0.5, 1.0, 0.5), (3.5, 1.0, 0.5), 0.0, 512, [(0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0)], False),
        # all three tMax tie at 1/4 and again at 3/4: x steps first, then y, then z, through cells of zero length
        ("through a cell corner", (0.5, 0.5, 0.5), (2.5, 2.5, 2.5), 0.0, 512,
         [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)], False),
        # floor(1.0) = 1: going down, the ray leaves its start cell at s = 0
        ("origin on a face, going down", (1.0, 0.5, 0.5), (-1.0, 0.5, 0.5), 0.0, 512, [(1, 0, 0), (0, 0, 0), (-1, 0, 0)], False),
        # going up, tMax = 1/2 and 1: the end x = 3.0 (cell 3) is never reached at s < 1
        ("origin on a face, going up", (1.0, 0.5, 0.5), (3.0, 0.5, 0.5), 0.0, 512, [(1, 0, 0), (2, 0, 0)], False),
        # tMax_x = 1/4, 3/4, 5/4; tMax_y = 1/2, 3/2
        ("negative coordinates", (-0.5, -0.5, -0.5), (-2.5, -1.5, -0.5), 0.0, 512,
         [(-1, -1, -1), (-2, -1, -1), (-2, -2, -1), (-3, -2, -1)], False),
        ("shorter than the margin", (0.5, 0.5, 0.5), (1.0, 0.5, 0.5), 1.0, 512, [], False),
        ("as long as the margin", (0.5, 0.5, 0.5), (1.5, 0.5, 0.5), 1.0, 512, [], False),
        ("zero length", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 0.0, 512, [], False),
        ("cut at max_steps", (0.5, 0.5, 0.5), (4.5, 0.5, 0.5), 1.0, 2, [(0, 0, 0), (1, 0, 0)], True),
        ("max_steps cells and the end in the last", (0.5, 0.5, 0.5), (4.5, 0.5, 0.5), 1.0, 4,
         [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)], False),
    ]


# ---- the traversal -------------------------------------------------------------------------------------------------------
def test_traversal_against_the_exact_oracle():
    """2 000 random rays: the cells the stepping visits are the cells the segment crosses with positive length, found from
    exact slab intersections.  A ray is left out where two crossing parameters lie within 1e-9 of each other or of s_end
    (there the rounded tMax may order two crossings the other way, or step once past the end): at most 1 %."""
    rng = np.random.default_rng(42)
    total = left_out = 0
    longest = 0
    for res in (1.0, 0.3):
        for spread in (2.0, 300.0):                                  # through the origin's neighbourhood, and far from it
            for _ in range(500):
                o = rng.uniform(-spread, spread, 3)
                v = rng.normal(size=3)
                q = o + v / np.linalg.norm(v) * rng.uniform(1.5, 8.0)
                got, cut, s_end = CR.traverse(o, q, res, res, max_steps=4096)
                assert not cut and s_end is not None
                want, cuts = CR.exact_cells(o, q, res, s_end)
                total += 1
                gaps = np.diff(np.array(cuts + [s_end]))
                if len(gaps) and gaps.min() < 1e-9:
                    left_out += 1
                    continue
                assert len(got) == len(set(got)) and set(got) == want, (res, o, q)
                longest = max(longest, len(got))
    print(f"rays {total}, left out {left_out}, most cells on a ray {longest}")
    assert total == 2000 and left_out == 0 and longest > 40


@pytest.mark.parametrize("ray", tie_rays(), ids=lambda r: r[0])
def test_hand_made_rays_follow_the_tie_rules(ray):
    _, o, q, margin, max_steps, cells, cut = ray
    got, got_cut, _ = CR.traverse(o, q, 1.0, margin, max_steps)
    assert got == cells and got_cut == cut


def test_bad_rays_are_not_cast():
    T = np.eye(4)
    T[:3, 3] = [0.5, 0.5, 0.5]
    pts = np.array([[1.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [2.0e6, 0.0, 0.0], [0.0, 0.0, -3.0]])
    assert list(CR.rays(pts, T, 1.0, 1.0)[3]) == [0, 4]
    T[0, 3] = 2.0e6                                                  # the sensor itself beyond the key range: no ray at all
    assert len(CR.rays(pts, T, 1.0, 1.0)[3]) == 0
    # a ray that would leave the key range ends there, without being cut
    got, cut, _ = CR.traverse((1048574.5, 0.5, 0.5), (1048575.5, 0.5, 0.5), 1.0, 0.0)
    assert got == [(1048574, 0, 0), (1048575, 0, 0)] and not cut


# ---- one Gaussian --------------------------------------------------------------------------------------------------------
def closest_sigma(m, cell, o, q):
    """the Mahalanobis distance of the line through o and q from the cell's mean: min over s, in closed form"""
    A6, mu = m["icov"][cell], m["mean"][cell]
    A = np.array([[A6[0], A6[1], A6[2]], [A6[1], A6[3], A6[4]], [A6[2], A6[4], A6[5]]])
    d, v = np.asarray(q) - np.asarray(o), np.asarray(o) - mu
    return float(np.sqrt(max(v @ A @ v - (d @ A @ v) ** 2 / (d @ A @ d), 0.0)))


def test_rays_against_a_hand_built_cell():
    hb, names = NR.hand_built_cells()
    m = UR.build(hb, 16)
    six = int(np.nonzero(m["keys"] == NR.cell_key(names["six"]))[0][0])
    mu = m["mean"][six].copy()
    assert m["valid"][six] and m["valid"].sum() == 2
    ex, ey = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    toward = 1.0 if mu[1] - np.floor(mu[1]) < 0.5 else -1.0          # the side on which the cell has more room
    unit = closest_sigma(m, six, mu - 2.5 * ex + ey, mu + 2.2 * ex + ey)   # sigmas per metre of offset along y

    def one(o, q, **kw):
        T = np.eye(4)
        T[:3, 3] = o
        info = CR.carve(m, (np.asarray(q) - T[:3, 3])[None], T, min_pass=1, miss_frames=100, **kw)
        assert info[0] == 1 and info[2] == 0
        return int(m["pass"][six]), int(m["hit"][six]), int(m["pass"].sum()), int(m["hit"].sum())

    # through the mean, ending 1.2 m behind it (end margin 1 of L = 4.7): passes, does not hit
    assert one(mu - 2.5 * ex, mu + 2.2 * ex) == (1, 0, 1, 0)
    # parallel to it: at 0.9 sigma it passes, at 1.1 sigma and at 5 sigma it does not
    for k, want in ((0.9, 1), (1.1, 0), (5.0, 0)):
        off = toward * (k / unit) * ey
        o, q = mu - 2.5 * ex + off, mu + 2.2 * ex + off
        assert abs(closest_sigma(m, six, o, q) - k) < 1e-9
        if k < 2.0:                                                  # still inside the cell's row: the cell is evaluated
            assert tuple(names["six"]) in CR.traverse(o, q, 1.0, 1.0)[0]
        assert one(o, q) == (want, 0, want, 0), k
    # ending in the cell: the walk stops one margin before the mean, in the cell in front: a hit and nothing else
    assert one(mu - 2.5 * ex, mu) == (0, 1, 0, 1)
    # ending in the cell in front of it, inside the margin: neither
    q = np.array([np.floor(mu[0]) - 0.1, mu[1], mu[2]])
    assert one(q - 2.0 * ex, q) == (0, 0, 0, 0)
    # the same ray without a margin walks up to its end and still does not reach the cell
    assert one(q - 2.0 * ex, q, end_margin=0.0) == (0, 0, 0, 0)
    # and one that ends just behind the cell's front face, without a margin, is evaluated over the short piece inside
    q = np.array([np.floor(mu[0]) + 0.01, mu[1], mu[2]])
    s6 = closest_sigma(m, six, q - 2.0 * ex, q)
    got = one(q - 2.0 * ex, q, end_margin=0.0)
    assert s6 < 1e-6 and got[1] == 1                                  # the line goes through the mean, the piece stops short of it
    A = m["icov"][six]
    assert got[0] == int(A[0] * (q[0] - mu[0]) ** 2 <= 1.0)          # decided at the piece's end, the clamped s*


# ---- the decision --------------------------------------------------------------------------------------------------------
def test_the_decision_rule_on_a_hand_made_table():
    rng = np.random.default_rng(7)
    mp = np.concatenate([np.array([float(c), 0.0, 0.0]) + 0.1 + 0.8 * rng.random((8, 3)) for c in range(7)] +
                        [np.array([[7.5, 0.5, 0.5]])])               # cells 0 .. 6 valid, cell 7 has one point
    m = UR.build(mp, 16)
    assert list(m["valid"]) == [True] * 7 + [False] and m["count"][7] == 1
    before = {k: np.array(m[k]).copy() for k in ("keys", "count", "mean", "icov", "valid", "S")}
    CR.state(m)
    #                      hit resets | too few | counts | clears | hit wins | invalid cell
    m["pass"][:] = [5, 0, 1, 2, 9, 9, 0, 9]
    m["hit"][:] = [1, 3, 0, 0, 0, 2, 0, 0]
    m["miss"][:] = [2, 1, 1, 0, 2, 2, 2, 2]
    assert CR.decide(m, min_pass=2, miss_frames=3) == (2, 1)
    assert list(m["miss"]) == [0, 0, 1, 1, 0, 0, 2, 2]
    assert list(m["count"]) == [8, 8, 8, 8, 0, 8, 8, 1] and list(m["valid"]) == [True] * 4 + [False] + [True] * 2 + [False]
    assert not m["mean"][4].any() and not m["icov"][4].any() and not m["S"][4].any()
    assert m["keys"].tobytes() == before["keys"].tobytes()            # the cleared cell keeps its key
    for k, a in before.items():                                       # every other cell keeps every bit
        keep = np.arange(8) != 4
        assert np.array(m[k])[keep].tobytes() == a[keep].tobytes(), k
    # the cleared cell is no longer live: passes do not count against it
    m["pass"][4], m["hit"][4] = 9, 0
    assert CR.decide(m, min_pass=2, miss_frames=3) == (1, 0) and m["miss"][4] == 0 and m["miss"][3] == 2


def test_a_closed_gate_changes_nothing():
    with_pole, _ = phantom_scene()
    m = UR.build(with_pole[::20], CAPACITY, min_points=3)
    pts = thinned(1)
    assert CR.carve(m, pts, T_TRUE, min_pass=1, miss_frames=2)[1] > 0   # some state to keep
    before = {k: np.array(m[k]).copy() for k in ("keys", "count", "mean", "icov", "valid", "S", "pass", "hit", "miss")}
    assert before["pass"].any() and before["hit"].any() and before["miss"].any()
    for gate in (2, 3, -1):
        assert CR.carve(m, pts[::2], T_TRUE, gate=gate, min_pass=1, miss_frames=2) == [0, 0, 0, 0]
        for k, a in before.items():
            assert np.array(m[k]).tobytes() == a.tobytes(), (gate, k)
    for gate in (0, 1):
        assert CR.carve(m, pts[::2], T_TRUE, gate=gate, min_pass=1, miss_frames=100)[0] == len(pts[::2])


# ---- the phantom scene ---------------------------------------------------------------------------------------------------
def test_the_phantom_is_cleared_after_three_frames_and_nothing_else_ever():
    with_pole, only = phantom_scene()
    m = UR.build(with_pole, CAPACITY)
    assert len(m["keys"]) == 2535 and len(only) == 2 and m["valid"][only].all()
    others = np.setdiff1d(np.arange(len(m["keys"])), only)
    n_valid = int(m["valid"][others].sum())
    start = {k: np.array(m[k]).copy() for k in ("count", "mean", "icov", "valid", "S")}
    for frame in (1, 2, 3):
        visited = []
        pts = thinned(frame)
        info = CR.carve(m, pts, T_TRUE, visited=visited)
        false_candidates = int((m["miss"][others] > 0).sum())
        print(f"frame {frame}: rays {info[0]}, seen through {info[1]}, cleared {info[2]}, cut {info[3]}, cells per ray "
              f"{np.mean(visited):.2f}, false candidates {false_candidates} of {n_valid}")
        assert info[0] == len(pts) and info[3] == 0
        assert false_candidates == 0 and info[1] == 2               # a condition, not a tolerance
        assert info[2] == (2 if frame == 3 else 0)
        assert (m["count"][only] == 0).all() == (frame == 3)
        for k, a in start.items():                                   # no other cell changes, ever
            assert np.array(m[k])[others].tobytes() == a[others].tobytes(), (frame, k)
    assert len(pts) and not m["valid"][only].any() and not m["mean"][only].any() and not m["S"][only].any()
    # a cleared cell that receives points again has the bits of a founded cell
    q = np.concatenate([thinned(4), LR.transform(phantom_pole()[:40], np.linalg.inv(T_TRUE))])
    UR.update(m, q, T_TRUE)
    assert (m["count"][only] > 0).all()
    fresh = UR.build(np.zeros((0, 3)), CAPACITY)
    UR.update(fresh, q, T_TRUE)
    for c in only:
        f = int(np.nonzero(fresh["keys"] == m["keys"][c])[0][0])
        for k in ("count", "mean", "S", "icov", "valid"):
            assert np.array(m[k][c]).tobytes() == np.array(fresh[k][f]).tobytes(), k
