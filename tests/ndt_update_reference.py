"""Independent numpy restatement of the online NDT map (include/sps_hip.h, "NDT localiser, online map").
It imports tests/ndt_reference.py (the static map and the alignment) and never touches the native library.  Every
floating-point operation is a float64 one rounded on its own, in the order the header states, so the kernels and this
file agree bit for bit: there is no exp on this path and no sum whose order is left open.

Two routes: ``update`` merges a frame into the stored moments as the header describes it; ``rebuild`` recomputes every
cell two-pass from all the points it has ever seen (``NR.cells`` on the union), the yardstick of the merge's rounding."""
import numpy as np

from tests import localiser_reference as LR
from tests import ndt_reference as NR

EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- moments and records -----------------------------------------------------------------------------------------------
def batch_moments(xyz, groups, order, start):
    """Per group g: (n, mean [3], S [6]) over xyz[order[start[g] : start[g + 1]]] in that order: the sum, the division,
    then the second pass of outer products (the operation order of NR.cells / k_ndt_cells)."""
    G = groups
    count = (start[1:] - start[:-1]).astype(np.int64)
    total = np.zeros((G, 3))
    for t in range(int(count.max()) if G else 0):
        on = count > t
        total[on] = total[on] + xyz[order[start[:-1][on] + t]]
    with np.errstate(all="ignore"):
        mean = np.where(count[:, None] > 0, total / np.maximum(count, 1)[:, None].astype(np.float64), 0.0)
    S = np.zeros((G, 6))
    for t in range(int(count.max()) if G else 0):
        on = count > t
        d = xyz[order[start[:-1][on] + t]] - mean[on]
        prod = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                         d[:, 2] * d[:, 2]], axis=1)
        S[on] = S[on] + prod
    return count, mean, S


def records(count, mean, S, min_points, eig_ratio):
    """(icov [C, 6], valid [C]) from the moments: S / (n - 1), 8 Jacobi sweeps, the eigenvalue floor, the inverse."""
    C = len(count)
    two = count >= 2
    cov = np.zeros((C, 6))
    cov[two] = S[two] / (count[two] - 1)[:, None].astype(np.float64)
    lam, vec = NR.jacobi(cov)
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
    return icov, valid


# ---- the dynamic map ---------------------------------------------------------------------------------------------------
def build(map_xyz, capacity, resolution=1.0, min_points=6, eig_ratio=0.01):
    """The dynamic map after sps_ndt_map_build_dynamic: the assigned cells in id order (ascending key for the cells of
    the build), dict(keys, count, mean, S, icov, valid, capacity, dropped, resolution, min_points, eig_ratio, seen)."""
    xyz = np.ascontiguousarray(np.asarray(map_xyz).reshape(-1, np.asarray(map_xyz).shape[-1])[:, :3], dtype=np.float64)
    keys, start, order = NR.group(xyz, resolution)
    if len(keys) > capacity or capacity < 1:
        raise ValueError("cell_capacity must be >= max(n_cells, 1)")
    count, mean, S = batch_moments(xyz, len(keys), order, start)
    icov, valid = records(count, mean, S, min_points, eig_ratio)
    return dict(keys=keys.copy(), count=count, mean=mean, S=S, icov=icov, valid=valid, capacity=int(capacity), dropped=0,
                resolution=float(resolution), min_points=int(min_points), eig_ratio=float(eig_ratio), seen=[xyz])


def update(m, pts, T, gate=None, max_cell_points=0, cap=None, n=None):
    """sps_ndt_map_update on the map ``m`` (changed in place).  Returns info = [cells assigned, founded, dropped, points
    integrated]."""
    if gate is not None and gate not in (0, 1):
        return [len(m["keys"]), 0, 0, 0]
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    cap = len(pts) if cap is None else int(cap)
    n = min(cap, max(len(pts) if n is None else int(n), 0))
    q = LR.transform(pts[:n], np.asarray(T, dtype=np.float64))
    res = m["resolution"]
    with np.errstate(invalid="ignore"):
        f = np.floor(q / res)
        ok = np.all((f >= -NR.KEY_LIMIT) & (f <= NR.KEY_LIMIT), axis=1)          # NaN and infinities compare false
    idx = np.nonzero(ok)[0]
    key = NR.cell_key(f[idx].astype(np.int64))
    # cells: the map's by key, then the founders in ascending founder index while ids last
    ids = {int(k): c for c, k in enumerate(m["keys"])}
    n0 = len(ids)
    founders, dropped = 0, set()
    cell = np.full(len(idx), -1, dtype=np.int64)
    new_keys = []
    for j, k in enumerate(key):                                                   # ascending point index
        k = int(k)
        if k in ids:
            cell[j] = ids[k]
        elif k not in dropped:
            if n0 + founders < m["capacity"]:
                ids[k] = n0 + founders
                cell[j] = ids[k]
                new_keys.append(k)
                founders += 1
            else:
                dropped.add(k)
    on = cell >= 0
    idx, cell = idx[on], cell[on]
    C = n0 + founders
    for name, width in (("mean", 3), ("S", 6), ("icov", 6)):
        m[name] = np.concatenate([m[name], np.zeros((founders, width))])
    m["keys"] = np.concatenate([m["keys"], np.array(new_keys, dtype=np.uint64)])
    m["count"] = np.concatenate([m["count"], np.zeros(founders, dtype=np.int64)])
    m["valid"] = np.concatenate([m["valid"], np.zeros(founders, dtype=bool)])
    m["dropped"] += len(dropped)
    m["seen"].append(q[idx])
    if len(idx):
        order = np.argsort(cell, kind="stable")                                   # ascending point index inside a cell
        tc, nb = np.unique(cell[order], return_counts=True)
        start = np.zeros(len(tc) + 1, dtype=np.int64)
        start[1:] = np.cumsum(nb)
        nb, mu_b, S_b = batch_moments(q[idx], len(tc), order, start)
        cnt, mu, S = m["count"][tc].copy(), m["mean"][tc].copy(), m["S"][tc].copy()
        mm = int(max_cell_points)
        if mm >= 2:
            forget = cnt > mm
            fac = np.float64(mm - 1) / (cnt[forget] - 1).astype(np.float64)
            S[forget] = S[forget] * fac[:, None]
            cnt[forget] = mm
        fresh = cnt == 0
        n2 = cnt + nb
        with np.errstate(all="ignore"):
            delta = mu_b - mu
            fr = nb.astype(np.float64) / n2.astype(np.float64)
            g = (cnt.astype(np.float64) * nb.astype(np.float64)) / n2.astype(np.float64)
            mu2 = mu + delta * fr[:, None]
            dd = np.stack([delta[:, 0] * delta[:, 0], delta[:, 0] * delta[:, 1], delta[:, 0] * delta[:, 2],
                           delta[:, 1] * delta[:, 1], delta[:, 1] * delta[:, 2], delta[:, 2] * delta[:, 2]], axis=1)
            S2 = (S + S_b) + dd * g[:, None]
        mu2[fresh], S2[fresh] = mu_b[fresh], S_b[fresh]
        icov, valid = records(n2, mu2, S2, m["min_points"], m["eig_ratio"])
        m["count"][tc], m["mean"][tc], m["S"][tc], m["icov"][tc], m["valid"][tc] = n2, mu2, S2, icov, valid
    return [C, founders, len(dropped), int(len(idx))]


def rebuild(m):
    """The second route: NR.cells over every point the map has taken, two-pass (no forgetting, no capacity)."""
    return NR.cells(np.concatenate(m["seen"]), m["resolution"], m["min_points"], m["eig_ratio"])


def as_cmap(m):
    """The assigned cells in ascending key order, in the form NR.hits / NR.align read (and NR.cells returns)."""
    o = np.argsort(m["keys"], kind="stable")
    return dict(keys=m["keys"][o], count=m["count"][o], mean=m["mean"][o], icov=m["icov"][o], valid=m["valid"][o],
                resolution=m["resolution"], rows=o)


def rows_by_capacity(m):
    """What sps_ndt_map_cells writes for the dynamic map: capacity rows, unassigned rows with count 0 and the empty key."""
    C, n = m["capacity"], len(m["keys"])
    keys = np.full(C, EMPTY_KEY, dtype=np.uint64)
    keys[:n] = m["keys"]
    out = dict(keys=keys)
    for name, width, dt in (("count", 0, np.int64), ("mean", 3, np.float64), ("icov", 6, np.float64), ("valid", 0, bool)):
        a = np.zeros((C, width) if width else C, dtype=dt)
        a[:n] = m[name]
        out[name] = a
    return out
