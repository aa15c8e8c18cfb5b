"""Independent numpy restatement of the NDT localiser (include/sps_hip.h, "NDT localiser"; DESIGN.md "NDT localiser").
It shares no code with sps_amd/localiser.py and never touches the native library.  As in tests/localiser_reference.py
every floating-point operation is a float64 one rounded on its own, in the order the header states, so the kernels and
this file agree term by term apart from exp (two libraries, each within its documented error); only the order in which
the per-cell terms are ADDED differs (here: one flat sequential sum over (point, lookup order), forward or reversed; on
the device: cells within a point, points within a workgroup, workgroups in block order)."""
import math

import numpy as np

from tests import localiser_reference as LR
from tests.localiser_reference import downsample, perturbation, pose_difference  # noqa: F401  (shared with the ICP's)

KEY_LIMIT = 1048575
SWEEPS = 8
# lookup order of the neighbourhood: the own cell, then +x, -x, +y, -y, +z, -z
OFFSETS = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.int64)
SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))                  # rows of a symmetric matrix stored (xx, xy, xz, yy, yz, zz)


# ---- the map -------------------------------------------------------------------------------------------------------------
def cell_index(xyz, resolution):
    """floor(v / resolution) per axis: negative coordinates floor, they do not truncate."""
    return np.floor(np.asarray(xyz, dtype=np.float64) / float(resolution)).astype(np.int64)


def cell_key(c):
    c = np.asarray(c, dtype=np.int64)
    return (((c[..., 2] + (1 << 20)) << 42) | ((c[..., 1] + (1 << 20)) << 21) | (c[..., 0] + (1 << 20))).astype(np.uint64)


def group(map_xyz, resolution):
    """(cell keys ascending, start [C + 1], map indices grouped by cell, ascending inside a cell)."""
    xyz = np.ascontiguousarray(np.asarray(map_xyz)[:, :3], dtype=np.float64)
    if len(xyz) == 0:
        return np.zeros(0, np.uint64), np.zeros(1, np.int64), np.zeros(0, np.int64)
    keys = cell_key(cell_index(xyz, resolution))
    order = np.argsort(keys, kind="stable")
    ukeys, counts = np.unique(keys[order], return_counts=True)
    start = np.zeros(len(ukeys) + 1, dtype=np.int64)
    start[1:] = np.cumsum(counts)
    return ukeys, start, order


def _rotate(a, v, p, q):
    """One Jacobi rotation zeroing a[:, p, q], vectorised over the cells; cells with a[p][q] == 0 are left alone."""
    r = 3 - p - q
    apq = a[:, p, q].copy()
    on = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
        t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        t = np.where(theta < 0.0, -t, t)
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        app = a[:, p, p] - t * apq
        aqq = a[:, q, q] + t * apq
        arp, arq = a[:, r, p].copy(), a[:, r, q].copy()
        nrp = c * arp - s * arq
        nrq = s * arp + c * arq
    a[:, p, p] = np.where(on, app, a[:, p, p])
    a[:, q, q] = np.where(on, aqq, a[:, q, q])
    a[:, p, q] = a[:, q, p] = np.where(on, 0.0, apq)
    a[:, r, p] = a[:, p, r] = np.where(on, nrp, arp)
    a[:, r, q] = a[:, q, r] = np.where(on, nrq, arq)
    for k in range(3):
        vkp, vkq = v[:, k, p].copy(), v[:, k, q].copy()
        with np.errstate(all="ignore"):
            v[:, k, p] = np.where(on, c * vkp - s * vkq, vkp)
            v[:, k, q] = np.where(on, s * vkp + c * vkq, vkq)


def jacobi(cov6):
    """[C, 6] symmetric matrices -> (eigenvalues [C, 3] = the diagonal after SWEEPS cyclic sweeps, eigenvectors [C, 3, 3]
    as columns)."""
    C = len(cov6)
    a = np.zeros((C, 3, 3))
    for i in range(3):
        for j in range(3):
            a[:, i, j] = cov6[:, SYM[i][j]]
    v = np.tile(np.eye(3), (C, 1, 1))
    for _ in range(SWEEPS):
        _rotate(a, v, 0, 1)
        _rotate(a, v, 0, 2)
        _rotate(a, v, 1, 2)
    return np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1), v


def cells(map_xyz, resolution=1.0, min_points=6, eig_ratio=0.01, route="jacobi"):
    """The device map: dict(keys, count, mean [C, 3], cov [C, 6], lam [C, 3] (floored eigenvalues), icov [C, 6], valid).
    route = "eigh" takes the eigen-decomposition from numpy.linalg.eigh instead (the tolerance's yardstick)."""
    xyz = np.ascontiguousarray(np.asarray(map_xyz)[:, :3], dtype=np.float64)
    keys, start, order = group(xyz, resolution)
    C = len(keys)
    count = (start[1:] - start[:-1]).astype(np.int64)
    rows = np.arange(C)
    total = np.zeros((C, 3))
    for t in range(int(count.max()) if C else 0):                    # sums in ascending order of the cell's list
        on = count > t
        total[on] = total[on] + xyz[order[start[:-1][on] + t]]
    with np.errstate(all="ignore"):
        mean = np.where(count[:, None] > 0, total / np.maximum(count, 1)[:, None].astype(np.float64), 0.0)
    cov = np.zeros((C, 6))
    for t in range(int(count.max()) if C else 0):
        on = count > t
        d = xyz[order[start[:-1][on] + t]] - mean[on]
        prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                         d[:, 2] * d[:, 2]], axis=1)
        cov[on] = cov[on] + prod
    two = count >= 2
    cov[two] = cov[two] / (count[two] - 1)[:, None].astype(np.float64)
    cov[~two] = 0.0
    if route == "eigh":
        full = np.zeros((C, 3, 3))
        for i in range(3):
            for j in range(3):
                full[:, i, j] = cov[:, SYM[i][j]]
        lam, vec = np.linalg.eigh(full) if C else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    else:
        lam, vec = jacobi(cov)
    lmax = lam.max(axis=1) if C else np.zeros(0)
    lfloor = float(eig_ratio) * lmax
    lam = np.where(lam < lfloor[:, None], lfloor[:, None], lam)
    icov = np.zeros((C, 6))
    with np.errstate(all="ignore"):
        k = 0
        for i in range(3):
            for j in range(i, 3):
                icov[:, k] = ((vec[:, i, 0] * vec[:, j, 0]) / lam[:, 0] + (vec[:, i, 1] * vec[:, j, 1]) / lam[:, 1]) + \
                             (vec[:, i, 2] * vec[:, j, 2]) / lam[:, 2]
                k += 1
    icov[~two] = 0.0
    valid = (count >= min_points) & two & (lmax > 0.0) & np.isfinite(mean).all(axis=1) & np.isfinite(icov).all(axis=1)
    return dict(keys=keys, count=count, mean=mean, cov=cov, lam=lam, icov=icov, valid=valid, resolution=float(resolution),
                rows=rows)


def gauss(outlier_ratio, resolution):
    """(d1, d2) of PCL's Gaussian fit of the uniform + normal mixture."""
    c1 = 10.0 * (1.0 - outlier_ratio)
    c2 = outlier_ratio / (resolution * resolution * resolution)
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    d2 = -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)
    return d1, d2


# ---- one iteration -------------------------------------------------------------------------------------------------------
def symrow(m6, i, b):
    """row i of the symmetric matrices m6 [m, 6] times the vectors b [m, 3], as (m0*b0 + m1*b1) + m2*b2"""
    r = SYM[i]
    return (m6[:, r[0]] * b[:, 0] + m6[:, r[1]] * b[:, 1]) + m6[:, r[2]] * b[:, 2]


def hits(q, cmap, neighbours, d1, d2):
    """Every contributing (point, cell) pair, ordered by point and then by lookup order.
    dict(i, c, terms [m, 28] (21 of H, 6 of g, the score), w, faces (points on a cell face), boundary (cells whose weight
    lies within 4 ulp of the guard's upper end; the lower end, 0, is inclusive and exp is never negative))."""
    res = cmap["resolution"]
    with np.errstate(invalid="ignore"):
        f = np.floor(q / res)
        ok = np.all((f >= -KEY_LIMIT) & (f <= KEY_LIMIT), axis=1)    # NaN compares false
    ids = np.nonzero(ok)[0]
    faces = int(np.sum(np.any(q[ids] / res == f[ids], axis=1)))
    base = f[ids].astype(np.int64)
    pi, pc, cell = [], [], []
    for c in range(neighbours):
        cc = base + OFFSETS[c]
        inr = np.all(np.abs(cc) <= KEY_LIMIT, axis=1)
        key = cell_key(cc)
        pos = np.searchsorted(cmap["keys"], key)
        pos = np.minimum(pos, max(len(cmap["keys"]) - 1, 0))
        found = inr & (cmap["keys"][pos] == key) if len(cmap["keys"]) else np.zeros(len(ids), bool)
        found = found & cmap["valid"][pos] if len(cmap["keys"]) else found
        pi.append(ids[found])
        pc.append(np.full(int(found.sum()), c))
        cell.append(pos[found])
    pi, pc, cell = np.concatenate(pi), np.concatenate(pc), np.concatenate(cell)
    order = np.lexsort((pc, pi))
    pi, pc, cell = pi[order], pc[order], cell[order]
    qq = q[pi]
    M = cmap["icov"][cell]
    x = qq - cmap["mean"][cell]
    y = np.stack([symrow(M, 0, x), symrow(M, 1, x), symrow(M, 2, x)], axis=1)
    s = LR.dot3(x, y)
    nd1 = -d1
    with np.errstate(all="ignore"):
        e = np.exp(-0.5 * (d2 * s))
        w = d2 * e
        keep = (w >= 0.0) & (w <= 1.0)
    boundary = int(np.sum(np.abs(w - 1.0) <= 4 * np.spacing(1.0)))
    pi, pc, qq, M, y, e, w = pi[keep], pc[keep], qq[keep], M[keep], y[keep], e[keep], w[keep]
    a = nd1 * w
    cols = LR.jacobian_columns(qq)
    u = [np.stack([symrow(M, 0, cols[c]), symrow(M, 1, cols[c]), symrow(M, 2, cols[c])], axis=1) for c in range(6)]
    out = [a * LR.dot3(cols[r], u[c]) for r in range(6) for c in range(r, 6)]
    out += [a * LR.dot3(cols[r], y) for r in range(6)]
    out.append(nd1 * e)
    terms = np.stack(out, axis=1) if len(pi) else np.zeros((0, 28))
    return dict(i=pi, c=pc, terms=terms, w=w, faces=faces, boundary=boundary)


def score(pts, cmap, T, neighbours=7, outlier_ratio=0.55):
    """sum over the contributing cells of -d1 exp(-d2 s / 2) at the pose T (math.fsum: the finite-difference test's f)."""
    d1, d2 = gauss(outlier_ratio, cmap["resolution"])
    h = hits(LR.transform(pts, np.asarray(T, dtype=np.float64)), cmap, neighbours, d1, d2)
    return math.fsum(h["terms"][:, 27]), h


def twist_pose(xi, T):
    """[Exp(omega), v; 0, 1] T for the twist xi = (omega, v): the left-multiplied update of the alignment."""
    E, _ = LR.exp_so3([float(v) for v in xi[:3]])
    return LR.left_multiply(E, [float(v) for v in xi[3:]], np.asarray(T, dtype=np.float64))


# ---- the whole alignment -------------------------------------------------------------------------------------------------
def align(pts, cmap, T_init, iters=30, neighbours=7, min_corr=50, outlier_ratio=0.55, tol_t=1e-4, tol_r=1e-5, reverse=False):
    """The whole call, with the outputs of localiser_reference.align: dict(pose, status, iterations, n_corr, trace [it, 4]
    = (points counted, score, |v|, |omega|), normal [it, 28] (b = -g), terms (per iteration, per contributing cell, with
    b's sign), faces, boundary (summed over the iterations))."""
    d1, d2 = gauss(outlier_ratio, cmap["resolution"])
    T0 = np.array(T_init, dtype=np.float64)
    T = T0.copy()
    status, trace, normal, all_terms, faces, boundary, n_corr = 1, [], [], [], 0, 0, 0
    it = 0
    for it in range(1, iters + 1):
        h = hits(LR.transform(pts, T), cmap, neighbours, d1, d2)
        faces += h["faces"]
        boundary += h["boundary"]
        terms = h["terms"]
        tot = LR.ordered_sum(terms, reverse)
        n_corr = len(np.unique(h["i"]))
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
        x = LR.cholesky_solve(tot)
        if x is None:
            status = 3
            break
        E, th = LR.exp_so3(x[:3])
        vn = math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5])
        T = LR.left_multiply(E, x[3:], T)
        trace[-1][2], trace[-1][3] = vn, th
        if vn < tol_t and th < tol_r:
            status = 0
            break
    if status in (2, 3):
        T = T0.copy()
    return dict(pose=T, status=status, iterations=it if iters else 0, n_corr=n_corr, trace=np.array(trace).reshape(-1, 4),
                normal=np.array(normal).reshape(-1, 28), terms=all_terms, faces=faces, boundary=boundary)


# ---- hand-built cells (shared by the CPU and the GPU tests) ---------------------------------------------------------------
def hand_built_cells(origin=(200.0, 200.0, 50.0)):
    """Map points that fill four cells of edge 1 far from anything else, and one at x < 0:
    five points (invalid: below min_points), six points (valid), six identical points (invalid: lambda_max = 0),
    six coplanar points (valid, smallest eigenvalue floored).  Returns (points [n, 3], dict name -> cell index triple)."""
    o = np.asarray(origin, dtype=np.float64)
    rng = np.random.default_rng(5)
    five = o + [0.0, 0.0, 0.0] + 0.1 + 0.8 * rng.random((5, 3))
    six = o + [3.0, 0.0, 0.0] + 0.1 + 0.8 * rng.random((6, 3))
    same = np.tile(o + [6.0, 0.0, 0.0] + [0.25, 0.5, 0.75], (6, 1))
    plane = o + [9.0, 0.0, 0.0] + 0.1 + 0.8 * rng.random((6, 3))
    plane[:, 2] = o[2] + 0.5                                           # z constant: the covariance has rank 2
    neg = np.array([[-0.3, 200.2, 50.4]])                              # resolution 1: cell (-1, 200, 50)
    pts = np.concatenate([five, six, same, plane, neg])
    names = dict(five=cell_index(five[0], 1.0), six=cell_index(six[0], 1.0), same=cell_index(same[0], 1.0),
                 plane=cell_index(plane[0], 1.0), neg=cell_index(neg[0], 1.0))
    return pts, names


def find_cell(cmap, c):
    """row of the cell with index triple c in a cells() dict"""
    pos = int(np.searchsorted(cmap["keys"], cell_key(np.asarray(c))))
    assert cmap["keys"][pos] == cell_key(np.asarray(c))
    return pos
