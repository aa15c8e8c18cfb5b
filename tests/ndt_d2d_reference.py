"""Independent numpy restatement of distribution-to-distribution NDT (include/sps_hip.h, "NDT localiser, distribution to
distribution").  It shares no code with sps_amd/localiser.py and never touches the native library.  As in
tests/ndt_reference.py every floating-point operation is a float64 one rounded on its own, in the order the header
states, so the kernels and this file agree term by term apart from exp; only the order in which the per-pair terms are
ADDED differs (here: one flat sequential sum over (source, lookup order), forward or reversed)."""
import math

import numpy as np

from tests import localiser_reference as LR
from tests import ndt_reference as NR
from tests.ndt_reference import KEY_LIMIT, OFFSETS, SYM, cell_key, gauss, jacobi, symrow

REC = 10                                                             # SPS_NDT_SRC_REC


# ---- the scan's cells ----------------------------------------------------------------------------------------------------
def _sequential(rows):
    """0.0 + rows[0] + rows[1] + ... down the first axis, one rounding per addition"""
    return np.add.accumulate(np.concatenate([np.zeros((1,) + rows.shape[1:]), rows]), axis=0)[-1]


def sources(pts, resolution, min_points=6, eig_ratio=0.01, route="jacobi"):
    """The source records of the points pts [n, 3] (sensor frame), in founder order: cell j is the j-th cell in ascending
    order of the lowest point index that falls in it.  dict(mean [C, 3], cov [C, 6], count, valid, first (that lowest
    index), lam [C, 3] (floored eigenvalues), scov [C, 6] (the sample covariance S / (n - 1) that was decomposed), n_src =
    (cells, valid cells), resolution).  route = "eigh" takes the
    eigen-decomposition from numpy.linalg.eigh instead (the tolerance's yardstick)."""
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    with np.errstate(all="ignore"):
        f = np.floor(pts / float(resolution))
        ok = np.all((f >= -KEY_LIMIT) & (f <= KEY_LIMIT), axis=1)    # NaN compares false, an infinite quotient fails too
        ok &= np.isfinite(pts).all(axis=1)
    ids = np.nonzero(ok)[0]
    keys = cell_key(f[ids].astype(np.int64)) if len(ids) else np.zeros(0, np.uint64)
    _, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                         # unique cells by their first point
    C = len(order)
    mean, S, count = np.zeros((C, 3)), np.zeros((C, 6)), np.zeros(C, np.int64)
    for j, u in enumerate(order):
        p = pts[ids[np.nonzero(inv == u)[0]]]                        # ascending point index
        n = len(p)
        mu = _sequential(p) / float(n)
        d = p - mu
        prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                         d[:, 2] * d[:, 2]], axis=1)
        mean[j], S[j], count[j] = mu, _sequential(prod), n
    two = count >= 2
    cv = np.zeros((C, 6))
    cv[two] = S[two] / (count[two] - 1)[:, None].astype(np.float64)
    if route == "eigh":
        full = np.zeros((C, 3, 3))
        for i in range(3):
            for j in range(3):
                full[:, i, j] = cv[:, SYM[i][j]]
        lam, vec = np.linalg.eigh(full) if C else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    else:
        lam, vec = jacobi(cv)
    lmax = lam.max(axis=1) if C else np.zeros(0)
    lfloor = float(eig_ratio) * lmax
    lam = np.where(lam < lfloor[:, None], lfloor[:, None], lam)
    cov = np.zeros((C, 6))
    k = 0
    for i in range(3):
        for j in range(i, 3):
            cov[:, k] = ((vec[:, i, 0] * vec[:, j, 0]) * lam[:, 0] + (vec[:, i, 1] * vec[:, j, 1]) * lam[:, 1]) + \
                        (vec[:, i, 2] * vec[:, j, 2]) * lam[:, 2]
            k += 1
    cov[~two] = 0.0
    valid = (count >= min_points) & two & (lmax > 0.0) & np.isfinite(mean).all(axis=1) & np.isfinite(cov).all(axis=1)
    return dict(mean=mean, cov=cov, count=count, valid=valid, first=ids[first[order]] if C else np.zeros(0, np.int64), lam=lam,
                scov=cv,
                n_src=(C, int(valid.sum())), resolution=float(resolution))


def hand_sources(mean, cov=None, valid=None):
    """a sources() dict from hand-made records (cov None: zero covariances; valid None: all valid)"""
    mean = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).reshape(-1, 3))
    C = len(mean)
    cov = np.zeros((C, 6)) if cov is None else np.ascontiguousarray(np.asarray(cov, dtype=np.float64).reshape(C, 6))
    valid = np.ones(C, bool) if valid is None else np.asarray(valid, dtype=bool)
    return dict(mean=mean, cov=cov, count=np.zeros(C, np.int64), valid=valid, n_src=(C, int(valid.sum())))


def records(src):
    """the device layout [C, REC] of a sources() dict"""
    return np.concatenate([src["mean"], src["cov"], src["valid"].astype(np.float64)[:, None]], axis=1)


def hand_built_points(origin=(20.0, 20.0, 5.0)):
    """Scan points (sensor frame) that fill cells of edge 1, modelled on ndt_reference.hand_built_cells: five points
    (invalid: below min_points), six (valid), six identical (invalid: lambda_max = 0), six coplanar (valid, floor exact),
    one at x < 0 (floor, not truncation), one exactly on a cell face (x = 30 belongs to cell 30).  Returns (points, dict
    name -> cell index triple); the points are interleaved, so founder order is not the order of the names."""
    o = np.asarray(origin, dtype=np.float64)
    rng = np.random.default_rng(7)
    five = o + 0.1 + 0.8 * rng.random((5, 3))
    six = o + [3.0, 0.0, 0.0] + 0.1 + 0.8 * rng.random((6, 3))
    same = np.tile(o + [6.0, 0.0, 0.0] + [0.25, 0.5, 0.75], (6, 1))
    plane = o + [9.0, 0.0, 0.0] + 0.1 + 0.8 * rng.random((6, 3))
    plane[:, 2] = o[2] + 0.5
    neg = np.array([[-0.3, 20.2, 5.4]])
    face = np.array([[30.0, 20.5, 5.5]])
    groups = dict(five=five, six=six, same=same, plane=plane, neg=neg, face=face)
    names = {k: NR.cell_index(v[0], 1.0) for k, v in groups.items()}
    allp = np.concatenate(list(groups.values()))
    perm = np.random.default_rng(11).permutation(len(allp))
    return allp[perm], names


def find_source(src, c):
    """row of the source cell with index triple c"""
    keys = cell_key(NR.cell_index(src["mean"], src["resolution"]))
    pos = np.nonzero(keys == cell_key(np.asarray(c)))[0]
    assert len(pos) == 1
    return int(pos[0])


# ---- one iteration -------------------------------------------------------------------------------------------------------
def inv3(m):
    """([m, 6] inverses by cofactors, ok [m]): det = (m0 c00 + m1 c01) + m2 c02, every entry c / det; ok is false where
    det <= 0 (NaN included) or an entry is not finite"""
    with np.errstate(all="ignore"):
        c00 = m[:, 3] * m[:, 5] - m[:, 4] * m[:, 4]
        c01 = m[:, 2] * m[:, 4] - m[:, 1] * m[:, 5]
        c02 = m[:, 1] * m[:, 4] - m[:, 2] * m[:, 3]
        c11 = m[:, 0] * m[:, 5] - m[:, 2] * m[:, 2]
        c12 = m[:, 1] * m[:, 2] - m[:, 0] * m[:, 4]
        c22 = m[:, 0] * m[:, 3] - m[:, 1] * m[:, 1]
        det = (m[:, 0] * c00 + m[:, 1] * c01) + m[:, 2] * c02
        out = np.stack([c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det], axis=1)
    return out, (det > 0.0) & np.isfinite(out).all(axis=1)


def rotate_cov(cov6, R):
    """Cw = R C R^T of the symmetric matrices cov6 [m, 6] -> [m, 6]: U = R C first, every entry (a0 b0 + a1 b1) + a2 b2,
    then Cw = U R^T the same way"""
    U = [[(R[i, 0] * cov6[:, SYM[0][j]] + R[i, 1] * cov6[:, SYM[1][j]]) + R[i, 2] * cov6[:, SYM[2][j]] for j in range(3)]
         for i in range(3)]
    return np.stack([(U[i][0] * R[j, 0] + U[i][1] * R[j, 1]) + U[i][2] * R[j, 2] for i in range(3) for j in range(i, 3)], axis=1)


def hits(src, cmap, T, neighbours, d1, d2, R_frozen=None):
    """Every contributing (source, map cell) pair at the pose T, ordered by source and then by lookup order.
    dict(i (source row), c, terms [m, 28] (21 of H, 6 of g, the score), w, faces (sources whose q lies on a cell face),
    boundary (pairs whose weight lies within 4 ulp of the guard's upper end)).  R_frozen: the rotation that turns the
    source covariances instead of T's (the finite-difference test's frozen B)."""
    T = np.asarray(T, dtype=np.float64)
    rows = np.nonzero(src["valid"])[0]
    q = LR.transform(src["mean"][rows], T)
    Cw = rotate_cov(src["cov"][rows], T[:3, :3] if R_frozen is None else np.asarray(R_frozen, dtype=np.float64))
    res = cmap["resolution"]
    with np.errstate(invalid="ignore"):
        f = np.floor(q / res)
        ok = np.all((f >= -KEY_LIMIT) & (f <= KEY_LIMIT), axis=1)
    ids = np.nonzero(ok)[0]
    faces = int(np.sum(np.any(q[ids] / res == f[ids], axis=1)))
    base = f[ids].astype(np.int64)
    pi, pc, cell = [], [], []
    nk = len(cmap["keys"])
    for c in range(neighbours):
        cc = base + OFFSETS[c]
        inr = np.all(np.abs(cc) <= KEY_LIMIT, axis=1)
        key = cell_key(np.where(inr[:, None], cc, 0))
        pos = np.minimum(np.searchsorted(cmap["keys"], key), max(nk - 1, 0))
        found = (inr & (cmap["keys"][pos] == key) & cmap["valid"][pos]) if nk else np.zeros(len(ids), bool)
        pi.append(ids[found])
        pc.append(np.full(int(found.sum()), c))
        cell.append(pos[found])
    pi, pc, cell = np.concatenate(pi), np.concatenate(pc), np.concatenate(cell)
    order = np.lexsort((pc, pi))
    pi, pc, cell = pi[order], pc[order], cell[order]
    qq = q[pi]
    Sm, ok1 = inv3(cmap["icov"][cell])
    B, ok2 = inv3(Sm + Cw[pi])
    x = qq - cmap["mean"][cell]
    with np.errstate(all="ignore"):
        y = np.stack([symrow(B, 0, x), symrow(B, 1, x), symrow(B, 2, x)], axis=1)
        s = LR.dot3(x, y)
        e = np.exp(-0.5 * (d2 * s))
        w = d2 * e
        keep = ok1 & ok2 & (w >= 0.0) & (w <= 1.0)
    boundary = int(np.sum(np.abs(w[ok1 & ok2] - 1.0) <= 4 * np.spacing(1.0)))
    pi, pc, qq, B, y, e, w = pi[keep], pc[keep], qq[keep], B[keep], y[keep], e[keep], w[keep]
    nd1 = -d1
    a = nd1 * w
    cols = LR.jacobian_columns(qq)
    u = [np.stack([symrow(B, 0, cols[c]), symrow(B, 1, cols[c]), symrow(B, 2, cols[c])], axis=1) for c in range(6)]
    out = [a * LR.dot3(cols[r], u[c]) for r in range(6) for c in range(r, 6)]
    out += [a * LR.dot3(cols[r], y) for r in range(6)]
    out.append(nd1 * e)
    terms = np.stack(out, axis=1) if len(pi) else np.zeros((0, 28))
    return dict(i=rows[pi], c=pc, terms=terms, w=w, faces=faces, boundary=boundary)


def score(src, cmap, T, neighbours=7, outlier_ratio=0.55, R_frozen=None):
    """sum over the contributing pairs of -d1 exp(-d2 s / 2) at the pose T (math.fsum), and the hits"""
    d1, d2 = gauss(outlier_ratio, cmap["resolution"])
    h = hits(src, cmap, T, neighbours, d1, d2, R_frozen)
    return math.fsum(h["terms"][:, 27]), h


# ---- the whole alignment -------------------------------------------------------------------------------------------------
def align(src, cmap, T_init, iters=30, neighbours=7, min_corr=50, outlier_ratio=0.55, tol_t=1e-4, tol_r=1e-5, reverse=False):
    """The whole call, with the outputs of ndt_reference.align; n_corr and trace[:, 0] count sources."""
    d1, d2 = gauss(outlier_ratio, cmap["resolution"])
    T0 = np.array(T_init, dtype=np.float64)
    T = T0.copy()
    status, trace, normal, all_terms, faces, boundary, n_corr = 1, [], [], [], 0, 0, 0
    it = 0
    for it in range(1, iters + 1):
        h = hits(src, cmap, T, neighbours, d1, d2)
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


# ---- an independently written D2D (matrix products, numpy.linalg.inv): the restatement's own yardstick ---------------------
def full3(m6):
    M = np.zeros((len(m6), 3, 3))
    for i in range(3):
        for j in range(3):
            M[:, i, j] = m6[:, SYM[i][j]]
    return M


def align_matrix(src, cmap, T_init, iters=30, neighbours=7, min_corr=50, outlier_ratio=0.55, tol_t=1e-4, tol_r=1e-5):
    """D2D with 3 x 3 matrices, numpy.linalg.inv / solve and matrix products: dict(pose, status, iterations, counts)"""
    d1, d2 = gauss(outlier_ratio, cmap["resolution"])
    T = np.array(T_init, dtype=np.float64)
    T0 = T.copy()
    Sigma = np.zeros((len(cmap["keys"]), 3, 3))
    Sigma[cmap["valid"]] = np.linalg.inv(full3(cmap["icov"][cmap["valid"]]))
    lut = {int(k): i for i, k in enumerate(cmap["keys"]) if cmap["valid"][i]}
    rows = np.nonzero(src["valid"])[0]
    mu, C = src["mean"][rows], full3(src["cov"][rows])
    status, counts, it = 1, [], 0
    for it in range(1, iters + 1):
        R, t = T[:3, :3], T[:3, 3]
        q = mu @ R.T + t
        Cw = R @ C @ R.T
        base = np.floor(q / cmap["resolution"]).astype(np.int64)
        H, g, counted = np.zeros((6, 6)), np.zeros(6), 0
        for s in range(len(rows)):
            any_ = False
            J = np.zeros((3, 6))
            J[:, 3:] = np.eye(3)
            J[:, :3] = -np.array([[0, -q[s, 2], q[s, 1]], [q[s, 2], 0, -q[s, 0]], [-q[s, 1], q[s, 0], 0]])
            for k in range(neighbours):
                cc = base[s] + OFFSETS[k]
                if np.any(np.abs(cc) > KEY_LIMIT):
                    continue
                pos = lut.get(int(cell_key(cc)))
                if pos is None:
                    continue
                B = np.linalg.inv(Sigma[pos] + Cw[s])
                x = q[s] - cmap["mean"][pos]
                y = B @ x
                w = d2 * math.exp(-0.5 * d2 * float(x @ y))
                if not 0.0 <= w <= 1.0:
                    continue
                H += (-d1 * w) * (J.T @ B @ J)
                g += (-d1 * w) * (J.T @ y)
                any_ = True
            counted += any_
        counts.append(counted)
        if counted < min_corr:
            status = 2
            break
        x = np.linalg.solve(H, -g)
        T = NR.twist_pose(x, T)
        if np.linalg.norm(x[3:]) < tol_t and np.linalg.norm(x[:3]) < tol_r:
            status = 0
            break
    if status == 2:
        T = T0
    return dict(pose=T, status=status, iterations=it if iters else 0, counts=counts)
