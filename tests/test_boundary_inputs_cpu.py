"""The hand-built inputs of tests/boundary_inputs.py keep their teeth: every property the GPU tests of
tests/test_hip_boundaries.py rely on is asserted here, on the CPU, not assumed."""
import math

import numpy as np
import pytest

from tests import boundary_inputs as BI
from tests import localiser_reference as LR
from tests import ndt_reference as NR


# ---- the lattice set -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice_counts():
    """per cell size: (scan values on which floor(v / c) and floor(v * (1 / c)) differ, brute-force hits,
    hits lost by the reciprocal lookup, hits lost with division on both sides)"""
    out = {}
    for c in BI.LATTICE_CELLS:
        pts = BI.lattice(c)
        differ = int(np.sum(BI.floor_div(pts, c) != BI.floor_mul(pts, c)))
        hits, lost_mul = BI.lost_hits(pts, pts, c, c, BI.floor_mul)
        _, lost_div = BI.lost_hits(pts, pts, c, c, BI.floor_div)
        out[c] = (differ, hits, lost_mul, lost_div)
        print(f"lattice c = {c}: {len(pts)} points, floors differ on {differ} values, {hits} hits, "
              f"lost by floor(v * (1 / c)): {lost_mul}, lost by floor(v / c): {lost_div}")
    return out


def test_lattice_shape():
    for c in BI.LATTICE_CELLS:
        pts = BI.lattice(c)
        assert pts.shape == (3 * (2 * BI.LATTICE_K + 1), 3) and len(np.unique(pts, axis=0)) == len(pts) - 0
        k = np.arange(-BI.LATTICE_K, BI.LATTICE_K + 1)
        assert np.array_equal(pts[:len(k), 0], k * c)                  # k * c itself, not an accumulated sum
        off = pts[:len(k), 1:]
        assert (BI.floor_div(off, c) == 0).all() and (BI.floor_mul(off, c) == 0).all()   # the offsets: cell 0 either way


@pytest.mark.parametrize("c", [0.7, 1.3])
def test_reciprocal_lookup_loses_hits_on_the_lattice(lattice_counts, c):
    differ, hits, lost_mul, lost_div = lattice_counts[c]
    assert differ > 0 and hits > len(BI.lattice(c))                    # every point hits itself, and more
    assert lost_mul >= 1
    assert lost_div == 0


def test_lattice_at_a_tenth(lattice_counts):
    differ, hits, lost_mul, lost_div = lattice_counts[0.1]
    assert differ > 0
    assert lost_div == 0
    assert lost_mul == LOST_AT_A_TENTH                                  # recorded, whatever it is


LOST_AT_A_TENTH = 0


def test_the_issue_s_two_pairs_are_in_the_set():
    for c, k in ((0.7, 45), (1.3, 85)):
        q, m = k * c, (k + 1) * c
        assert (m - q) * (m - q) <= c * c
        assert math.floor(q * (1.0 / c)) == k - 1 and math.floor(m / c) == k + 1
        row = k + BI.LATTICE_K
        assert BI.lattice(c)[row, 0] == q and BI.lattice(c)[row + 1, 0] == m


def test_float32_lattice_keeps_hits_but_not_the_faces():
    """the float32 scan of the GPU test: promoted, it is 1e-8 (relative) off the lattice, so it checks the float path of the
    kernel, not the face rule"""
    for c in BI.LATTICE_CELLS:
        pts = BI.lattice(c)
        q = pts.astype(np.float32).astype(np.float64)
        hits, lost = BI.lost_hits(q, pts, c, c, BI.floor_div)
        assert hits > len(pts) // 2 and lost == 0


@pytest.mark.parametrize("c", BI.LATTICE_CELLS)
def test_lattice_split_shows_a_lost_hit_in_the_icp(c):
    scan, mp = BI.lattice_split(c)
    assert len(scan) == 900 and len(mp) == 903
    a = BI.nearest(scan, mp, c)
    i_div, j_div = BI.nearest_by_lookup(scan, mp, c, c, BI.floor_div)
    i_mul, j_mul = BI.nearest_by_lookup(scan, mp, c, c, BI.floor_mul)
    assert np.array_equal(i_div, a["i"]) and np.array_equal(j_div, a["j"])
    changed = int(np.sum(j_mul != a["j"])) if np.array_equal(i_mul, a["i"]) else -1
    print(f"lattice split c = {c}: n_corr {len(a['i'])}, ties {a['ties']}, d2 == r*r {a['on_r']}, partners changed by "
          f"floor(v * (1 / c)): {changed}")
    assert a["ties"] > 100 and len(a["i"]) > 600
    if c != 0.1:
        assert changed >= 1


# ---- the dyadic set --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dy():
    return BI.dyadic()


def test_dyadic_coordinates(dy):
    q, m, kind = dy["q"], dy["map"], dy["kind"]
    assert len(q) == BI.DYADIC_N == 520 and all((kind == k).sum() == 104 for k in BI.DYADIC_KINDS)
    assert np.array_equal(q * 16, np.round(q * 16)) and np.abs(q).max() < 64
    off = np.any(m * 16 != np.round(m * 16), axis=1)
    assert off.sum() == 104 and np.abs(m).max() < 64                   # the "beyond" points alone are off the 2^-4 grid
    assert (q < 0).any(axis=0).all() and (q == np.floor(q)).any(axis=0).all()   # negative coordinates, points on a face
    for t in BI.DYADIC_SHIFTS:
        p = q - np.asarray(t)
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p) and np.abs(p).max() < 64
        assert np.array_equal(LR.transform(p, BI.pose_of(t)), q)       # the pose brings the scan back, exactly


def test_dyadic_ties_boundaries_and_partners(dy):
    q, m, kind, want = dy["q"], dy["map"], dy["kind"], dy["want"]
    a = BI.nearest(q, m, BI.DYADIC_R)
    print(f"dyadic: n_corr {len(a['i'])}, ties {a['ties']}, d2 == r*r {a['on_r']}, one ulp beyond {a['beyond']}")
    assert a["ties"] == 104 and a["on_r"] == 104 and a["beyond"] == 104
    assert len(a["i"]) == 312 and np.array_equal(a["i"], np.nonzero(want >= 0)[0])
    assert np.array_equal(a["j"], want[want >= 0])
    d2 = BI.d2_matrix(q, m)
    assert len(dy["tie_pairs"]) == 104
    upper = 0
    for i, lo, hi in dy["tie_pairs"]:
        assert lo < hi and d2[i, lo] == d2[i, hi] <= 1.0 and want[i] == lo
        assert np.sum(d2[i] <= 1.0) == 2
        assert np.array_equal(q[i] - m[lo], -(q[i] - m[hi]))           # the residual flips sign with the partner
        upper += int(m[lo][np.nonzero(m[lo] != m[hi])[0][0]] > m[hi][np.nonzero(m[lo] != m[hi])[0][0]])
    assert 20 < upper < 84                                             # the lower index is on either side
    for i in np.nonzero(kind == "near")[0]:
        js = np.nonzero(d2[i] <= 1.0)[0]
        assert len(js) == 2 and want[i] == js.max() and d2[i, js.max()] < d2[i, js.min()]   # the nearer one has the higher index
    for i in np.nonzero(kind == "on_r")[0]:
        assert d2[i, want[i]] == 1.0 and np.sum(d2[i] <= 1.0) == 1
    for i in np.nonzero((kind == "beyond") | (kind == "none"))[0]:
        assert not (d2[i] <= 1.0).any()
    # the shared restatement's own association agrees when it is handed every pair
    b = LR.associate(q, BI.AllPairs(m, BI.DYADIC_R))
    assert np.array_equal(a["i"], b["i"]) and np.array_equal(a["j"], b["j"]) and b["ties"] == 104


def test_dyadic_sums_are_exact(dy):
    for n in (BI.DYADIC_N, 257, 33):
        for t in BI.DYADIC_SHIFTS:
            n_corr, terms, _ = BI.icp_terms(dy["q"][:n] - np.asarray(t), dy["map"], BI.DYADIC_R, BI.pose_of(t))
            assert n_corr == len(terms) > 0
            for k in range(28):
                exact = math.fsum(terms[:, k])
                assert exact == float(LR.ordered_sum(terms[:, k:k + 1])[0]) == float(LR.ordered_sum(terms[:, k:k + 1], reverse=True)[0])
            e = BI.exact_normal(terms)
            assert np.count_nonzero(e[21:27]) == 6 and e[27] > 0       # a wrong tie partner or boundary shows in b


def test_a_wrong_rule_changes_the_dyadic_sums(dy):
    """ties to the HIGHER index, or a strict d2 < r*r, or a bound one ulp wider, each change n_corr or b"""
    q, m = dy["q"], dy["map"]
    _, terms, a = BI.icp_terms(q, m, BI.DYADIC_R, np.eye(4))
    good = BI.exact_normal(terms)
    flipped = m[::-1]                                                   # the same points, index order reversed
    _, terms_f, _ = BI.icp_terms(q, flipped, BI.DYADIC_R, np.eye(4))
    assert not np.array_equal(BI.exact_normal(terms_f)[21:27], good[21:27])
    assert len(BI.nearest(q, m, math.nextafter(1.0, 0.0))["i"]) == len(a["i"]) - 104
    assert len(BI.nearest(q, m, 1.0 + 2.0 ** -40)["i"]) == len(a["i"]) + 104


# ---- the NDT inputs --------------------------------------------------------------------------------------------------------
def test_cell_pattern_is_valid_and_centred():
    cm = NR.cells(BI.cell_points([(0, 0, 0), (-3, 2, -1)]), 1.0)
    assert cm["valid"].all() and (cm["count"] == 8).all()
    assert np.array_equal(cm["mean"], np.array([[0.5, 0.5, 0.5], [-2.5, 2.5, -0.5]])[np.argsort(NR.cell_key(np.array([[0, 0, 0], [-3, 2, -1]])))])
    assert (cm["lam"].min(axis=1) > 0.01 * cm["lam"].max(axis=1)).all()                # non-coplanar: nothing floored


def test_ndt_block_map_covers_every_dyadic_point(dy):
    cm = NR.cells(BI.ndt_block_map(dy["q"]), 1.0)
    d1, d2 = NR.gauss(0.55, 1.0)
    for nb in (7, 1):
        h = NR.hits(dy["q"], cm, nb, d1, d2)
        assert len(np.unique(h["i"])) == BI.DYADIC_N and h["faces"] > 50 and h["boundary"] == 0


def test_ndt_face_case_takes_the_branches_it_is_built_for():
    mp, q, names = BI.ndt_face_case()
    cm = NR.cells(mp, 1.0)
    assert cm["valid"].all() and len(cm["keys"]) == 68
    d1, d2 = NR.gauss(0.55, 1.0)
    at = {n: i for i, n in enumerate(names)}
    f = np.floor(q)
    assert f[at["limit+x"], 0] == BI.KEY_LIMIT and f[at["limit-x"], 0] == -BI.KEY_LIMIT and f[at["limit face"], 0] == BI.KEY_LIMIT
    assert f[at["beyond+x"], 0] == BI.KEY_LIMIT + 1 and f[at["beyond-x"], 0] == -BI.KEY_LIMIT - 1
    h7, h1 = NR.hits(q, cm, 7, d1, d2), NR.hits(q, cm, 1, d1, d2)
    assert h7["faces"] == 9 and h7["boundary"] == 0
    per7 = {n: sorted(h7["c"][h7["i"] == i].tolist()) for n, i in at.items()}
    per1 = {n: sorted(h1["c"][h1["i"] == i].tolist()) for n, i in at.items()}
    assert per7["origin"] == per7["face-x"] == per7["corner-"] == [0, 1, 2, 3, 4, 5, 6]
    assert per7["face+x"] == [0, 2, 3, 4, 5, 6]                                           # floor(1.0) = 1: the last cell of the block
    assert per7["outer face"] == [0, 1, 3, 4, 5, 6] and per7["just outside"] == [2]       # floor(-2.0) = -2, floor(2.0) = 2
    assert per7["limit+x"] == [2] and per7["limit-x"] == [1] and per7["limit+y"] == [4] and per7["limit-z"] == [5]
    assert per7["limit face"] == [2]
    assert per7["beyond+x"] == per7["beyond-x"] == per7["beyond face"] == []               # one cell beyond: nothing
    assert all(per1[n] == [] for n in names if n.startswith(("limit", "beyond", "just")))
    assert per1["origin"] == per1["face-x"] == [0]


# ---- thinning --------------------------------------------------------------------------------------------------------------
def test_thinning_rows_take_the_branches_they_are_built_for():
    rows = BI.thinning_rows()
    keep, xyz = LR.downsample(rows, len(rows), 0.5)
    assert keep.tolist() == [0, 2, 4, 5, 8, 9, 12, 16]
    assert np.signbit(rows[5, 0]) and rows[5, 0] == 0.0
    v = np.floor(rows[:, :3].astype(np.float64) / 0.5)
    assert np.abs(v[keep]).max() == BI.KEY_LIMIT and (np.abs(v).max(axis=1)[[11, 14, 15, 17, 18]] == BI.KEY_LIMIT + 1).all()
    for n in (1023, 2049):
        fill = BI.thinning_fill(n)
        k, _ = LR.downsample(fill, n, 0.5)
        assert 0.5 * n < len(k) < 0.95 * n
