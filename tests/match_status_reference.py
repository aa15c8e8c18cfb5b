"""Independent numpy restatement of the scan-matching status (include/sps_hip.h, "localiser, scan-matching status";
DESIGN.md 8n).  It shares no code with sps_amd/localiser.py.  Every floating-point operation is a float64 one rounded on
its own, in the order the header states: the nearest map point by brute force over ALL map points with the kernel's d2
expression and tie rule (the device looks at 27 cells; within max_distance <= cell both see the same points), the sum of the
inliers' d2 in the device's two stages, the two true divisions and the verdict table."""
import math

import numpy as np

KEY_LIMIT = 1048575.0
LOC_PTS, LOC_SEG = 32, 8
LOST = 4
CHUNK = 64


def transform(pts, T):
    """q = R p + t as ((r0 * x + r1 * y) + r2 * z) + t, elementwise"""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def nearest(q, map_xyz, cell):
    """(d2 [n], j [n]) of the nearest map point of every q: d2 = (ex*ex + ey*ey) + ez*ez, ties to the lowest map index;
    (inf, -1) for an empty map and for a q that is not finite or whose cell floor(q / cell) leaves the key range"""
    n = len(q)
    d2, j = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    m = np.ascontiguousarray(map_xyz, dtype=np.float64)
    if n == 0 or len(m) == 0:
        return d2, j
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(q / np.float64(cell))
        ok = np.all((c >= -KEY_LIMIT) & (c <= KEY_LIMIT), axis=1)       # NaN and infinities compare false
    for s in range(0, n, CHUNK):
        ids = np.nonzero(ok[s:s + CHUNK])[0] + s
        if len(ids) == 0:
            continue
        e = q[ids][:, None, :] - m[None, :, :]
        dd = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
        k = np.argmin(dd, axis=1)                                         # the first minimum: the lowest map index
        d2[ids], j[ids] = dd[np.arange(len(ids)), k], k
    return d2, j


def nearest_within(q, map_xyz, cell, r, tree):
    """``nearest`` for the q that have a map point with d2 <= r * r, (inf, -1) for the others, in less time: ``tree`` (a
    scipy cKDTree of map_xyz) only narrows the candidates to a ball with a margin; the kernel's expression and the tie rule
    decide among them.  Which points are inliers, and their d2 and j, are those of ``nearest``."""
    n = len(q)
    d2, j = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    m = np.ascontiguousarray(map_xyz, dtype=np.float64)
    if n == 0 or len(m) == 0:
        return d2, j
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(q / np.float64(cell))
        ok = np.all((c >= -KEY_LIMIT) & (c <= KEY_LIMIT), axis=1)
    r2 = np.float64(r) * np.float64(r)
    ids = np.nonzero(ok)[0]
    for i, cand in zip(ids, tree.query_ball_point(q[ids], float(r) * (1.0 + 1e-6) + 1e-9)):
        if not cand:
            continue
        cand = np.sort(np.asarray(cand, dtype=np.int64))
        e = q[i] - m[cand]
        dd = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        k = int(np.argmin(dd))                                            # candidates ascending: the lowest map index
        if dd[k] <= r2:
            d2[i], j[i] = dd[k], cand[k]
    return d2, j


def two_stage_sum(values, inlier, n):
    """the inliers' values added as the device adds them: every run of LOC_PTS points in point order, the runs' rows in
    LOC_SEG runs of consecutive rows, each in order, then those in order"""
    nb = (n + LOC_PTS - 1) // LOC_PTS
    rows = []
    for b in range(nb):
        s = 0.0
        for i in range(b * LOC_PTS, min(n, (b + 1) * LOC_PTS)):
            if inlier[i]:
                s = s + float(values[i])
        rows.append(s)
    per = (nb + LOC_SEG - 1) // LOC_SEG
    total = 0.0
    for g in range(LOC_SEG):
        s = 0.0
        for b in range(g * per, min(nb, (g + 1) * per)):
            s = s + rows[b]
        total = total + s
    return total


def verdict(gate_in, n_valid, fraction, error, min_inlier_fraction, max_error, min_valid):
    """gate_in None: no gate word (0).  A word outside {0, 1} as an unsigned number passes through"""
    g = 0 if gate_in is None else int(gate_in)
    if g < 0 or g > 1:
        return g
    return g if (n_valid >= min_valid and fraction >= min_inlier_fraction and error <= max_error) else LOST


def status(pts, n_dev, cap, T, map_xyz, cell, max_distance=0.5, max_range=None, min_inlier_fraction=0.0, max_error=math.inf,
           min_valid=1, gate_in=None, tree=None):
    """``tree``: None for the brute-force search, or a cKDTree of map_xyz to narrow it (``nearest_within``).
    -> dict(inlier_fraction, matching_error, sum_d2, verdict, n_valid, n_inliers, n, d2 [n] as d2_dev holds it, j [n])"""
    n = min(int(cap), max(int(n_dev), 0))
    p = np.ascontiguousarray(np.asarray(pts, dtype=np.float64)[:n].reshape(n, 3))
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(p).all(axis=1)
        if max_range is not None and max_range >= 0:
            r2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
            valid &= r2 <= np.float64(max_range) * np.float64(max_range)
        q = transform(p, T)
    d2, j = nearest(q, map_xyz, cell) if tree is None else nearest_within(q, map_xyz, cell, max_distance, tree)
    md2 = np.float64(max_distance) * np.float64(max_distance)
    inlier = valid & (j >= 0) & (d2 <= md2)
    n_valid, n_in = int(valid.sum()), int(inlier.sum())
    total = two_stage_sum(d2, inlier, n)
    fraction = np.float64(n_in) / np.float64(max(n_valid, 1))
    error = np.float64(total) / np.float64(n_in) if n_in > 0 else np.float64(np.inf)
    out = np.where(inlier, d2, np.where(valid, np.inf, -1.0))
    return dict(inlier_fraction=float(fraction), matching_error=float(error), sum_d2=float(total),
                verdict=verdict(gate_in, n_valid, fraction, error, min_inlier_fraction, max_error, min_valid), n_valid=n_valid,
                n_inliers=n_in, n=n, d2=out, j=np.where(inlier, j, -1))


def out_bytes(r) -> bytes:
    """the 48 bytes of out_dev: double (inlier_fraction, matching_error, sum_d2, 0) | int32 (verdict, n_valid, n_inliers, n)"""
    return (np.array([r["inlier_fraction"], r["matching_error"], r["sum_d2"], 0.0], dtype=np.float64).tobytes()
            + np.array([r["verdict"], r["n_valid"], r["n_inliers"], r["n"]], dtype=np.int32).tobytes())
