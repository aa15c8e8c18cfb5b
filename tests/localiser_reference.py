"""Independent numpy restatement of the scan-to-map localiser (include/sps_hip.h, "localiser"; DESIGN.md "Localiser").
It shares no code with sps_amd/localiser.py.  Every floating-point operation is a float64 one rounded on its own
(numpy ufuncs and Python floats never contract a multiply and an add), in the order the header states, so the kernels
and this file agree term by term; only the order in which the per-point terms are ADDED differs (here: one flat
sequential sum, forward or reversed; on the device: per-workgroup partial rows added in block order)."""
import math

import numpy as np

KEY_LIMIT = 1048575.0
ASSOC_CHUNK = 2048


# ---- voxel-grid thinning -------------------------------------------------------------------------------------------------
def downsample(rows, n, leaf, cap=None):
    """rows [n_max, >=3] float32, the first n valid -> (surviving row indices ascending, their float64 (x, y, z))."""
    xyz = np.asarray(rows)[:n, :3].astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        v = np.floor(xyz / float(leaf))
        ok = np.all((v >= -KEY_LIMIT) & (v <= KEY_LIMIT), axis=1)       # NaN compares false: the row is skipped
    idx = np.nonzero(ok)[0]
    if len(idx) == 0:
        return idx, np.zeros((0, 3))
    _, first = np.unique(v[idx].astype(np.int64), axis=0, return_index=True)
    keep = np.sort(idx[first])                                           # lowest row index of every voxel, ascending
    if cap is not None:
        keep = keep[:cap]
    return keep, xyz[keep]


# ---- association ---------------------------------------------------------------------------------------------------------
def transform(pts, T):
    """q = R p + t as ((r0 * x + r1 * y) + r2 * z) + t, elementwise."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


class MapIndex:
    """Candidate narrowing only: a KD-tree ball query with a margin.  The winner is decided by the exact expression."""

    def __init__(self, map_xyz, r):
        from scipy.spatial import cKDTree
        self.xyz = np.ascontiguousarray(np.asarray(map_xyz)[:, :3], dtype=np.float64)
        self.r = float(r)
        self.tree = cKDTree(self.xyz) if len(self.xyz) else None

    def candidates(self, q):
        """(point index, map index) pairs of every candidate within r plus a margin."""
        fin = np.isfinite(q).all(axis=1)
        if self.tree is None or not fin.any():
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        ids = np.nonzero(fin)[0]
        lists = self.tree.query_ball_point(q[ids], self.r * (1.0 + 1e-6) + 1e-9)
        cnt = np.array([len(l) for l in lists], dtype=np.int64)
        pi = np.repeat(ids, cnt)
        mj = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if cnt.sum() else np.zeros(0, np.int64)
        return pi, mj


def associate(q, index: MapIndex):
    """Nearest map point of every q within r: d2 = (ex*ex + ey*ey) + ez*ez <= r*r, ties to the lowest map index.
    Returns dict(i, j, e, d2, ties, boundary): ties = points whose best and second-best d2 are equal, boundary = candidate
    pairs with |d2 - r2| <= 4 ulp."""
    if len(q) > ASSOC_CHUNK:                                             # bounded memory: the points are independent
        parts = [associate(q[s:s + ASSOC_CHUNK], index) for s in range(0, len(q), ASSOC_CHUNK)]
        out = {k: np.concatenate([p[k] + (s * ASSOC_CHUNK if k == "i" else 0) for s, p in enumerate(parts)])
               for k in ("i", "j", "e", "d2")}
        out.update(ties=sum(p["ties"] for p in parts), boundary=sum(p["boundary"] for p in parts))
        return out
    r2 = index.r * index.r
    pi, mj = index.candidates(q)
    e = q[pi] - index.xyz[mj]
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    boundary = int(np.sum(np.abs(d2 - r2) <= 4 * np.spacing(r2)))
    ok = d2 <= r2
    pi, mj, e, d2 = pi[ok], mj[ok], e[ok], d2[ok]
    order = np.lexsort((mj, d2, pi))                                     # by point, then d2, then map index
    pi, mj, e, d2 = pi[order], mj[order], e[order], d2[order]
    first = np.ones(len(pi), dtype=bool)
    first[1:] = pi[1:] != pi[:-1]
    second = np.zeros(len(pi), dtype=bool)
    second[1:] = first[:-1] & ~first[1:]
    ties = int(np.sum(d2[second] == d2[np.nonzero(second)[0] - 1])) if second.any() else 0
    return dict(i=pi[first], j=mj[first], e=e[first], d2=d2[first], ties=ties, boundary=boundary)


# ---- normal equations ----------------------------------------------------------------------------------------------------
def jacobian_columns(q):
    """The six columns of J = [ -[q]x | I ], each as its three residual-row entries [m, 3]."""
    z, o = np.zeros(len(q)), np.ones(len(q))
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    return [np.stack(c, axis=1) for c in ((z, -qz, qy), (qz, z, -qx), (-qy, qx, z), (o, z, z), (z, o, z), (z, z, o))]


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normal_terms(q, e, d2):
    """[m, 28] per-point terms: the 21 upper-triangle entries of J^T J (row-major), the 6 of J^T e, d2."""
    cols = jacobian_columns(q)
    out = [dot3(cols[r], cols[c]) for r in range(6) for c in range(r, 6)]
    out += [dot3(cols[r], e) for r in range(6)]
    out.append(d2)
    return np.stack(out, axis=1) if len(q) else np.zeros((0, 28))


def ordered_sum(terms, reverse=False):
    """Flat sequential sum of the rows (np.add.accumulate adds one row after the other)."""
    if len(terms) == 0:
        return np.zeros(terms.shape[1])
    t = terms[::-1] if reverse else terms
    return np.add.accumulate(t, axis=0)[-1]


# ---- solve and update ----------------------------------------------------------------------------------------------------
def cholesky_solve(tot):
    """H delta = b from the 28 sums (b = -g).  Returns delta (6 floats) or None for a pivot <= 0 / a non-finite solve."""
    H = [[0.0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i][j] = H[j][i] = float(tot[k])
            k += 1
    b = [-float(tot[21 + i]) for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = H[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d > 0.0:
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            s = H[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x if all(math.isfinite(v) for v in x) else None


def exp_so3(w):
    """Rodrigues: I + a K + c K^2 with a = sin(th) / th, c = 2 sin^2(th / 2) / th^2; first order below |w| < 1e-12."""
    wx, wy, wz = w
    th2 = (wx * wx + wy * wy) + wz * wz
    th = math.sqrt(th2)
    a, c = 1.0, 0.0
    if th >= 1e-12:
        sh = math.sin(0.5 * th)
        a = math.sin(th) / th
        c = (2.0 * (sh * sh)) / th2
    K = [[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]]
    E = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j]
            E[i][j] = ((1.0 if i == j else 0.0) + a * K[i][j]) + c * k2
    return E, th


def left_multiply(E, v, T):
    out = np.array(T, dtype=np.float64)
    for i in range(3):
        for j in range(4):
            s = (E[i][0] * float(T[0, j]) + E[i][1] * float(T[1, j])) + E[i][2] * float(T[2, j])
            if j == 3:
                s = s + v[i]
            out[i, j] = s
    return out


def align(pts, index: MapIndex, T_init, iters=30, min_corr=50, tol_t=1e-4, tol_r=1e-5, reverse=False):
    """The whole call.  dict(pose, status, iterations, n_corr, trace [it, 4], normal [it, 28], terms (per iteration: the
    [n_corr, 28] per-point terms with b's sign applied), ties, boundary (summed over the iterations))."""
    T0 = np.array(T_init, dtype=np.float64)
    T = T0.copy()
    status, trace, normal, all_terms, ties, boundary, n_corr = 1, [], [], [], 0, 0, 0
    it = 0
    for it in range(1, iters + 1):
        q = transform(pts, T)
        a = associate(q, index)
        ties += a["ties"]
        boundary += a["boundary"]
        terms = normal_terms(q[a["i"]], a["e"], a["d2"])
        tot = ordered_sum(terms, reverse)
        n_corr = len(a["i"])
        signed = terms.copy()
        signed[:, 21:27] *= -1.0
        all_terms.append(signed)
        row = tot.copy()
        row[21:27] *= -1.0
        normal.append(row)
        trace.append([float(n_corr), float(tot[27]), 0.0, 0.0])
        if n_corr < min_corr:
            status = 2
            break
        x = cholesky_solve(tot)
        if x is None:
            status = 3
            break
        E, th = exp_so3(x[:3])
        vn = math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5])
        T = left_multiply(E, x[3:], T)
        trace[-1][2], trace[-1][3] = vn, th
        if vn < tol_t and th < tol_r:
            status = 0
            break
    if status in (2, 3):
        T = T0.copy()
    return dict(pose=T, status=status, iterations=it if iters else 0, n_corr=n_corr, trace=np.array(trace).reshape(-1, 4),
                normal=np.array(normal).reshape(-1, 28), terms=all_terms, ties=ties, boundary=boundary)


# ---- helpers for the tests -------------------------------------------------------------------------------------------------
def perturbation(dx, dy, dz, yaw_deg, pitch_deg=0.0):
    a, p = math.radians(yaw_deg), math.radians(pitch_deg)
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
    Ry = np.array([[math.cos(p), 0, math.sin(p)], [0, 1.0, 0], [-math.sin(p), 0, math.cos(p)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry
    T[:3, 3] = [dx, dy, dz]
    return T


def pose_difference(A, B):
    """(translation distance, rotation angle in radians) between two poses."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    R = A[:3, :3].T @ B[:3, :3]
    s = np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3])), float(math.atan2(s, (np.trace(R) - 1.0) / 2.0))
