"""Hand-built inputs on which the documented rules of the radius grid and the localisers decide the result (ties to the
lowest map index, the inclusive d2 <= r*r, floor on a cell face, at negative coordinates and at the key limit), with
brute-force float64 references.  No GPU, no native library.

Association here is ALL PAIRS: no cell, no tree, no margin, so the references share no cell rule with the device.  The
only code shared with tests/localiser_reference.py is the arithmetic of one term (normal_terms / jacobian_columns), the
6 x 6 solve and the pose update."""
import math

import numpy as np

from tests import localiser_reference as LR
from tests import ndt_reference as NR

LATTICE_CELLS = (0.1, 0.7, 1.3)
LATTICE_K = 300
LATTICE_OFFSETS = (0.37, 0.61)            # the two other coordinates, in cells: well inside cell 0 under either rule
KEY_LIMIT = 1048575


# ---- all-pairs association -------------------------------------------------------------------------------------------------
def d2_matrix(q, m):
    """[n, M] d2 = (ex*ex + ey*ey) + ez*ez, e = q - m, every operation a float64 one rounded on its own"""
    q, m = np.asarray(q, dtype=np.float64), np.asarray(m, dtype=np.float64)
    ex = q[:, None, 0] - m[None, :, 0]
    ey = q[:, None, 1] - m[None, :, 1]
    ez = q[:, None, 2] - m[None, :, 2]
    return (ex * ex + ey * ey) + ez * ez


def hit_lists(q, m, r, chunk=512):
    """per query point, the ascending map indices with d2 <= r*r"""
    r2 = float(r) * float(r)
    out = []
    for s in range(0, len(q), chunk):
        ok = d2_matrix(q[s:s + chunk], m) <= r2
        out += [np.nonzero(row)[0] for row in ok]
    return out


def nearest(q, m, r, chunk=512):
    """The nearest map point of every q with d2 <= r*r, ties to the lowest map index (argmin returns the first minimum).
    dict(i, j, e, d2, ties (points whose two smallest d2 are equal), on_r (candidate pairs with d2 == r*r), beyond
    (candidate pairs with r*r < d2 <= r*r (1 + 2^-40)))"""
    q, m = np.asarray(q, dtype=np.float64), np.asarray(m, dtype=np.float64)
    r2 = float(r) * float(r)
    pi, pj, ties, on_r, beyond = [], [], 0, 0, 0
    for s in range(0, len(q), chunk):
        d2 = d2_matrix(q[s:s + chunk], m)
        on_r += int(np.sum(d2 == r2))
        beyond += int(np.sum((d2 > r2) & (d2 <= r2 * (1.0 + 2.0 ** -40))))
        d2 = np.where(d2 <= r2, d2, np.inf)
        j = np.argmin(d2, axis=1) if d2.shape[1] else np.zeros(len(d2), np.int64)
        best = d2[np.arange(len(d2)), j] if d2.shape[1] else np.full(len(d2), np.inf)
        has = np.isfinite(best)
        ties += int(np.sum(has & (np.sum(d2 == best[:, None], axis=1) > 1)))
        pi.append(s + np.nonzero(has)[0])
        pj.append(j[has])
    i = np.concatenate(pi) if pi else np.zeros(0, np.int64)
    j = np.concatenate(pj) if pj else np.zeros(0, np.int64)
    e = q[i] - m[j]
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return dict(i=i, j=j, e=e, d2=d2, ties=ties, on_r=on_r, beyond=beyond)


def icp_terms(pts, m, r, T):
    """One ICP iteration by brute force: (n_corr, [n_corr, 28] per-point terms as the device adds them: H, g, d2)"""
    q = LR.transform(np.asarray(pts, dtype=np.float64), np.asarray(T, dtype=np.float64))
    a = nearest(q, m, r)
    return len(a["i"]), LR.normal_terms(q[a["i"]], a["e"], a["d2"]), a


def exact_normal(terms):
    """The 28 `normal` entries from the per-point terms by math.fsum: H, b = -g, sum d2 (the negation is exact and a zero
    sum is +0.0 on either side, so b's zero is -0.0 as the device's is)"""
    tot = [math.fsum(terms[:, k]) for k in range(28)]
    return np.array(tot[:21] + [-v for v in tot[21:27]] + tot[27:], dtype=np.float64)


class AllPairs:
    """localiser_reference.align's `index` without an index: every (point, map point) pair is a candidate"""

    def __init__(self, map_xyz, r):
        self.xyz = np.ascontiguousarray(np.asarray(map_xyz)[:, :3], dtype=np.float64)
        self.r = float(r)

    def candidates(self, q):
        ids = np.nonzero(np.isfinite(q).all(axis=1))[0]
        return np.repeat(ids, len(self.xyz)), np.tile(np.arange(len(self.xyz)), len(ids))


# ---- the lattice set -------------------------------------------------------------------------------------------------------
def lattice(c, k_max=LATTICE_K):
    """[3 (2 k_max + 1), 3] float64: k * c on each axis in turn, the two other coordinates a fixed in-cell offset"""
    k = np.arange(-k_max, k_max + 1).astype(np.float64) * float(c)
    o1, o2 = LATTICE_OFFSETS[0] * float(c), LATTICE_OFFSETS[1] * float(c)
    rows = []
    for axis in range(3):
        p = np.empty((len(k), 3))
        p[:, axis] = k
        p[:, (axis + 1) % 3] = o1
        p[:, (axis + 2) % 3] = o2
        rows.append(p)
    return np.concatenate(rows)


def floor_div(v, c):
    return np.floor(np.asarray(v, dtype=np.float64) / float(c)).astype(np.int64)


def floor_mul(v, c):
    return np.floor(np.asarray(v, dtype=np.float64) * (1.0 / float(c))).astype(np.int64)


def lost_hits(q, m, r, cell, query_rule, map_rule=floor_div):
    """A model of the 27-cell lookup: the map is grouped by map_rule, the query's cell comes from query_rule; a brute-force
    hit whose map cell is more than one cell from the query's on some axis is never visited.  -> (hits, lost)"""
    cq, cm = query_rule(q, cell), map_rule(m, cell)
    hits = lost = 0
    for i, js in enumerate(hit_lists(q, m, r)):
        hits += len(js)
        lost += int(np.sum(np.any(np.abs(cm[js] - cq[i]) > 1, axis=1)))
    return hits, lost


def lattice_split(c, k_max=LATTICE_K):
    """(scan, map) for the ICP: the lattice's odd k as the scan, its even k as the map IN DESCENDING ORDER.  With scan ==
    map every point's partner would be itself at d2 = 0 and a lost hit at distance r could not show; here the partners of
    k * c are (k - 1) * c and (k + 1) * c, both at distance r up to rounding, and the farther-along one has the lower map
    index, so losing it changes the partner and the sign of e."""
    pts = lattice(c, k_max)
    odd = np.tile(np.arange(-k_max, k_max + 1) % 2 == 1, 3)
    return pts[odd], pts[~odd][::-1].copy()


def nearest_by_lookup(q, m, r, cell, query_rule, map_rule=floor_div):
    """nearest() under the model of lost_hits: only map points in the 27 cells around the query's cell are candidates.
    -> (i, j)"""
    r2 = float(r) * float(r)
    cq, cm = query_rule(q, cell), map_rule(m, cell)
    d2 = d2_matrix(q, m)
    seen = np.all(np.abs(cq[:, None, :] - cm[None, :, :]) <= 1, axis=2)
    d2 = np.where((d2 <= r2) & seen, d2, np.inf)
    j = np.argmin(d2, axis=1)
    has = np.isfinite(d2[np.arange(len(q)), j])
    return np.nonzero(has)[0], j[has]


# ---- the dyadic set --------------------------------------------------------------------------------------------------------
DYADIC_N = 520
DYADIC_KINDS = ("near", "tie", "on_r", "beyond", "none")
DYADIC_R = 1.0
TIE_OFFSETS = ((0.5, 0.0, 0.0), (0.0, 0.5, 0.0), (0.0, 0.0, 0.5), (0.25, 0.5, 0.0), (0.5, 0.25, 0.75))


def dyadic():
    """dict(q [520, 3], map [M, 3], kind [520], want [520] (map index of the wanted partner, -1 for none), tie_pairs).
    q is the scan IN THE MAP FRAME (the scan handed to the localiser is q - t for a pose of translation t).  Every q and
    every map point that can be chosen has coordinates that are multiples of 2^-4 with |v| < 64, so every product and sum
    of the ICP terms is exact in float64.  Point i is of kind DYADIC_KINDS[i % 5], its site 4 m from every other:
      near    two map points within r, the farther one at the lower map index
      tie     two map points at q + o and q - o: equal d2, the residual e = q - m flips sign between them
      on_r    one map point at distance exactly r along an axis (d2 == r*r)
      beyond  one map point one ulp beyond r along an axis -- the only coordinates that are not multiples of 2^-4, and
              they must never be chosen
      none    no map point within 3 m
    The map is shuffled, so a map index says nothing about the place or the cell order."""
    rng = np.random.default_rng(20240607)
    # |site| >= 4 on every axis: a "beyond" point then has |v| >= 2, where one ulp is >= 2^-52 and q - m is exact
    line = [v for v in range(-56, 57, 4) if v]
    sites = np.array([(x, y, z) for z in (-8, -4, 4, 8) for y in line for x in line], dtype=np.float64)
    sites = sites[rng.permutation(len(sites))[:DYADIC_N]]
    q = sites + rng.integers(0, 16, size=(DYADIC_N, 3)) / 16.0            # 0: on a cell face of the r = 1 grid
    kind = np.array([DYADIC_KINDS[i % 5] for i in range(DYADIC_N)])
    pts, owner, role = [], [], []
    for i in range(DYADIC_N):
        g = i // 5
        axis, sign = g % 3, 1.0 if (g // 3) % 2 == 0 else -1.0
        unit = np.zeros(3)
        unit[axis] = sign
        if kind[i] == "near":
            pts += [q[i] + sign * np.array([0.5, 0.5, 0.5]), q[i] + sign * np.array([0.25, -0.5, 0.125])]
            role += ["far", "want"]
        elif kind[i] == "tie":
            o = np.array(TIE_OFFSETS[g % len(TIE_OFFSETS)])
            pts += [q[i] + o, q[i] - o]
            role += ["tie", "tie"]
        elif kind[i] == "on_r":
            pts += [q[i] + DYADIC_R * unit]
            role += ["want"]
        elif kind[i] == "beyond":
            p = q[i] + DYADIC_R * unit
            p[axis] = np.nextafter(p[axis], sign * np.inf)
            pts += [p]
            role += ["beyond"]
        owner += [i] * (len(pts) - len(owner))
    pts, owner, role = np.array(pts), np.array(owner), np.array(role)
    # the shuffle; then "near" keeps its farther point at the lower index (swap where the shuffle says otherwise)
    perm = rng.permutation(len(pts))
    pts, owner, role = pts[perm], owner[perm], role[perm]
    for i in np.nonzero(kind == "near")[0]:
        far, want = np.nonzero((owner == i) & (role == "far"))[0][0], np.nonzero((owner == i) & (role == "want"))[0][0]
        if far > want:
            pts[[far, want]] = pts[[want, far]]
            role[[far, want]] = role[[want, far]]
    want = np.full(DYADIC_N, -1)
    tie_pairs = []
    for i in range(DYADIC_N):
        mine = np.nonzero(owner == i)[0]
        if kind[i] in ("near", "on_r"):
            want[i] = mine[role[mine] == "want"][0]
        elif kind[i] == "tie":
            want[i] = mine.min()
            tie_pairs.append((i, int(mine.min()), int(mine.max())))
    return dict(q=q, map=pts, kind=kind, want=want, tie_pairs=tie_pairs)


DYADIC_SHIFTS = ((0.0, 0.0, 0.0), (1.5, -2.25, 0.0625), (-3.0625, 0.5, 7.75))    # translations, multiples of 2^-4


def pose_of(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


# ---- the NDT maps ----------------------------------------------------------------------------------------------------------
# eight non-coplanar points inside a unit cell, multiples of 2^-4; eight of them, so the mean is exact: (0.5, 0.5, 0.5)
CELL_PATTERN = np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.3125], [0.25, 0.75, 0.375], [0.75, 0.75, 0.1875],
                         [0.25, 0.1875, 0.75], [0.75, 0.3125, 0.8125], [0.25, 0.8125, 0.6875], [0.75, 0.6875, 0.625]])


def cell_points(cells):
    """the pattern in every cell (resolution 1) of the integer triples `cells`"""
    c = np.asarray(cells, dtype=np.float64).reshape(-1, 3)
    return (c[:, None, :] + CELL_PATTERN[None, :, :]).reshape(-1, 3)


def ndt_block_map(q):
    """a valid cell under every point of q and at its six face neighbours (resolution 1; floor, also for a q on a face or
    at a negative coordinate)"""
    own = np.floor(q).astype(np.int64)
    return cell_points(np.unique((own[:, None, :] + NR.OFFSETS[None, :, :]).reshape(-1, 3), axis=0))


def ndt_face_case():
    """(map points, q [n, 3], names): scan points in the map frame on faces, at the key limit and one cell beyond it"""
    block = [(x, y, z) for x in range(-2, 2) for y in range(-2, 2) for z in range(-2, 2)]
    far = [(KEY_LIMIT - 1, 0, 0), (-(KEY_LIMIT - 1), 0, 0), (0, KEY_LIMIT - 1, 0), (0, 0, -(KEY_LIMIT - 1))]
    q = [("face+x", (1.0, 0.5, 0.25)), ("face-x", (-1.0, -0.5, 0.25)), ("face-y", (0.25, -1.0, 0.5)), ("face+z", (0.5, 0.25, 1.0)),
         ("origin", (0.0, 0.0, 0.0)), ("corner-", (-1.0, -1.0, -1.0)), ("inside", (0.4375, -0.5625, 0.3125)),
         ("outer face", (-2.0, 0.5, 0.5)), ("just outside", (2.0, 0.5, 0.5)),
         ("limit+x", (KEY_LIMIT + 0.5, 0.5, 0.5)), ("limit-x", (-KEY_LIMIT + 0.5, 0.5, 0.5)),
         ("limit+y", (0.5, KEY_LIMIT + 0.5, 0.5)), ("limit-z", (0.5, 0.5, -KEY_LIMIT + 0.5)),
         ("limit face", (float(KEY_LIMIT), 0.5, 0.5)), ("beyond+x", (KEY_LIMIT + 1.5, 0.5, 0.5)),
         ("beyond-x", (-KEY_LIMIT - 0.5, 0.5, 0.5)), ("beyond face", (float(KEY_LIMIT + 1), 0.5, 0.5))]
    return cell_points(block + far), np.array([v for _, v in q], dtype=np.float64), [n for n, _ in q]


# ---- thinning edges --------------------------------------------------------------------------------------------------------
def thinning_rows(leaf=0.5):
    """float32 rows for sps_loc_downsample at leaf 0.5 (exact in float32 and float64, so v / leaf is exact): rows on a voxel
    face with both signs, -0.0, the key limit and one voxel beyond it, and a second row in most voxels"""
    L = float(leaf)
    rows = [(1.0, 0.5, 0.25), (1.25, 0.5, 0.25),                      # face at +, then the same voxel again
            (-1.0, -0.5, 0.25), (-0.75, -0.5, 0.25),                  # face at -: voxel -2, and its second row
            (-1.25, -0.5, 0.25),                                      # voxel -3: below the face
            (-0.0, 0.125, 0.125), (0.0, 0.125, 0.125), (0.25, 0.125, 0.125),      # -0.0 is voxel 0, as +0.0 and 0.25 are
            (-0.25, 0.125, 0.125),                                        # voxel -1
            (KEY_LIMIT * L, 0.0, 0.0), ((KEY_LIMIT + 0.5) * L, 0.0, 0.0),          # voxel +1048575: kept once
            ((KEY_LIMIT + 1) * L, 0.0, 0.0),                                       # +1048576: skipped
            (-KEY_LIMIT * L, 0.0, 0.0), ((-KEY_LIMIT + 0.5) * L, 0.0, 0.0),        # voxel -1048575: kept once
            ((-KEY_LIMIT - 0.5) * L, 0.0, 0.0), ((-KEY_LIMIT - 1) * L, 0.0, 0.0),  # -1048576 twice: skipped
            (0.0, KEY_LIMIT * L, 0.0), (0.0, 0.0, (KEY_LIMIT + 1) * L), (0.0, (-KEY_LIMIT - 0.5) * L, 0.0)]
    out = np.array(rows, dtype=np.float32)
    assert np.array_equal(out.astype(np.float64), np.array(rows, dtype=np.float64))     # exact in float32
    return out


def thinning_fill(n, seed=3):
    """n float32 rows, multiples of 2^-3 in [-4, 4): 4096 voxels at leaf 0.5, every fourth coordinate on a voxel face, so
    a few hundred rows already share voxels with earlier ones"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-32, 32, size=(n, 3)) / 8.0).astype(np.float32)
