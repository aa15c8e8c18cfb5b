"""Independent numpy restatement of the online NDT map's free-space carving (include/sps_hip.h, "NDT localiser, online map:
free-space carving").  It works on the dict tests/ndt_update_reference.build returns, which gains the three
per-cell arrays ``pass``, ``hit`` and ``miss``, and never touches the native library.  Every floating-point operation is a
float64 one rounded on its own, in the order the header states; the results are integer counts and comparisons of such
doubles, so the kernels and this file agree exactly.

``steps`` is the traversal (Amanatides-Woo in the ray parameter s), ``carve`` the whole call.  ``exact_cells`` is a second,
independent route to the set of cells a segment crosses: exact slab intersections in ``fractions.Fraction``, no stepping."""
import math
from fractions import Fraction

import numpy as np

from tests import localiser_reference as LR
from tests import ndt_reference as NR

KEY_LIMIT = NR.KEY_LIMIT
INF = float("inf")


# ---- the rays ------------------------------------------------------------------------------------------------------------
def rays(pts, T, resolution, end_margin):
    """Origin o [3], ends q [m, 3], directions d = q - o, the indices (into pts) of the rays that are cast, the cell index
    triples of o and of every q, and s_end [m] (NaN: L <= end_margin, nothing is traversed)."""
    T = np.asarray(T, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):               # a bad row gives a bad end, which is then skipped
        q = LR.transform(pts, T)
    return rays_between(np.array([T[0, 3], T[1, 3], T[2, 3]]), q, resolution, end_margin)


def rays_between(o, q, resolution, end_margin):
    """``rays`` from the origin and the ends themselves"""
    with np.errstate(invalid="ignore", over="ignore"):
        fo = np.floor(o / resolution)
        fq = np.floor(q / resolution)
        ok_o = bool(np.isfinite(o).all() and np.all((fo >= -KEY_LIMIT) & (fo <= KEY_LIMIT)))
        ok = np.isfinite(q).all(axis=1) & np.all((fq >= -KEY_LIMIT) & (fq <= KEY_LIMIT), axis=1) & ok_o
    idx = np.nonzero(ok)[0]
    q = q[idx]
    d = q - o
    with np.errstate(all="ignore"):
        L = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        s_end = 1.0 - end_margin / L
    s_end = np.where(L <= end_margin, np.nan, s_end)
    co = fo.astype(np.int64) if ok_o else np.zeros(3, np.int64)
    return o, q, d, idx, co, fq[idx].astype(np.int64), s_end


def steps(o, d, co, s_end, resolution, max_steps):
    """The traversal of the rays (o, d[i]) over s in [0, s_end[i]), all rays in lockstep.  Yields per step
    (rows, cells [k, 3], s_in [k], s_out [k]) for the rays still running; after the last step ``cut`` (the generator's
    return value) flags the rays stopped at max_steps."""
    m = len(d)
    res = float(resolution)
    c = np.tile(np.asarray(co, dtype=np.int64), (m, 1))
    step = np.sign(d).astype(np.int64)
    with np.errstate(all="ignore"):
        edge = (c + (step > 0)).astype(np.float64) * res
        tmax = np.where(d != 0.0, (edge - o) / d, INF)
        tdelta = np.where(d != 0.0, res / np.abs(d), INF)
    s_in = np.zeros(m)
    on = ~np.isnan(s_end)
    cut = np.zeros(m, dtype=bool)
    done = 0
    while on.any():
        r = np.nonzero(on)[0]
        ax = np.argmin(tmax[r], axis=1)                              # the first of equal minima: the lowest axis
        t = tmax[r, ax]
        s_out = np.minimum(t, s_end[r])
        yield r, c[r].copy(), s_in[r].copy(), s_out
        done += 1
        go = ~(t >= s_end[r])
        if done >= max_steps:
            cut[r[go]] = True
            break
        r, ax, t = r[go], ax[go], t[go]
        c[r, ax] = c[r, ax] + step[r, ax]
        s_in[r] = t
        tmax[r, ax] = t + tdelta[r, ax]
        on[:] = False
        on[r[np.abs(c[r, ax]) <= KEY_LIMIT]] = True                  # a cell index leaving the key range ends the ray
    return cut


def traverse(o, q, resolution, end_margin, max_steps=512):
    """One ray from o to q: (the visited cell index triples in order, cut, s_end or None where nothing is traversed)."""
    o, q = np.asarray(o, dtype=np.float64), np.asarray(q, dtype=np.float64)
    _, _, d, idx, co, _, s_end = rays_between(o, q[None], resolution, end_margin)
    if len(idx) == 0:
        return [], False, None
    out = []
    gen = steps(o, d, co, s_end, resolution, max_steps)
    cut = None
    try:
        while True:
            _, cells, _, _ = next(gen)
            out.append(tuple(int(v) for v in cells[0]))
    except StopIteration as e:
        cut = e.value
    return out, bool(cut[0]) if cut is not None else False, None if np.isnan(s_end[0]) else float(s_end[0])


# ---- the exact oracle ----------------------------------------------------------------------------------------------------
def exact_cells(o, q, resolution, s_end):
    """The set of cells that the segment o + s (q - o), 0 <= s < s_end, crosses with positive length, and the sorted
    crossing parameters in (0, s_end): exact rational arithmetic on the doubles given, slab by slab, no stepping."""
    res = Fraction(float(resolution))
    fo = [Fraction(float(v)) for v in o]
    fd = [Fraction(float(b)) - Fraction(float(a)) for a, b in zip(o, q)]     # the exact difference of the two doubles
    se = Fraction(float(s_end))
    cuts = {Fraction(0), se}
    for a in range(3):
        if fd[a] == 0:
            continue
        lo, hi = sorted((fo[a], fo[a] + se * fd[a]))
        for k in range(math.ceil(lo / res), math.floor(hi / res) + 1):      # every plane k * res between the two ends
            s = (k * res - fo[a]) / fd[a]
            if 0 < s < se:
                cuts.add(s)
    cuts = sorted(cuts)
    cells = set()
    for s0, s1 in zip(cuts, cuts[1:]):
        mid = (s0 + s1) / 2
        cells.add(tuple(math.floor((fo[a] + mid * fd[a]) / res) for a in range(3)))
    return cells, [float(s) for s in cuts[1:-1]]


# ---- one carve -----------------------------------------------------------------------------------------------------------
def state(m):
    """the three per-cell arrays of the map, grown with zeros to the cells it has now"""
    C = len(m["keys"])
    for name in ("pass", "hit", "miss"):
        a = m.get(name, np.zeros(0, dtype=np.int64))
        m[name] = np.concatenate([a, np.zeros(C - len(a), dtype=np.int64)])
    return m["pass"], m["hit"], m["miss"]


def lookup(m, cells):
    """ids of the cells with the index triples ``cells`` [k, 3] (all inside the key range), -1 where the map has none"""
    if len(m["keys"]) == 0:
        return np.full(len(cells), -1, dtype=np.int64)
    order = np.argsort(m["keys"], kind="stable")
    skeys = m["keys"][order]
    key = NR.cell_key(cells)
    pos = np.minimum(np.searchsorted(skeys, key), len(skeys) - 1)
    return np.where(skeys[pos] == key, order[pos], -1)


def passes(m, cell, o, d, s_in, s_out, sigma2):
    """whether the rays (o, d[i]) pass through the Gaussians of the valid cells ``cell`` [k] over [s_in, s_out]"""
    A, mu = m["icov"][cell], m["mean"][cell]
    with np.errstate(all="ignore"):
        y = np.stack([NR.symrow(A, 0, d), NR.symrow(A, 1, d), NR.symrow(A, 2, d)], axis=1)
        a = LR.dot3(d, y)
        w = mu - o
        b = LR.dot3(y, w)
        s = b / a
        bad = ~(a > 0.0) | np.isnan(s)
        s = np.minimum(np.maximum(s, s_in), s_out)
        x = (o + s[:, None] * d) - mu
        z = np.stack([NR.symrow(A, 0, x), NR.symrow(A, 1, x), NR.symrow(A, 2, x)], axis=1)
        l = LR.dot3(x, z)
        return ~bad & (l <= sigma2)


def carve(m, pts, T, gate=None, end_margin=None, through_sigma=1.0, min_pass=2, miss_frames=3, max_steps=512, cap=None, n=None,
          visited=None):
    """sps_ndt_map_carve on the map ``m`` (changed in place).  Returns info = [rays cast, cells seen through, cells
    cleared, rays cut at max_steps].  ``visited`` (a list): gets the number of cells every cast ray visited."""
    cnt_pass, cnt_hit, miss = state(m)
    if gate is not None and gate not in (0, 1):
        return [0, 0, 0, 0]
    res = m["resolution"]
    end_margin = res if end_margin is None else float(end_margin)
    sigma2 = float(through_sigma) * float(through_sigma)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    cap = len(pts) if cap is None else int(cap)
    n = min(cap, max(len(pts) if n is None else int(n), 0))
    o, q, d, idx, co, cq, s_end = rays(pts[:n], T, res, end_margin)
    cnt_pass[:] = 0
    cnt_hit[:] = 0
    ends = lookup(m, cq)
    np.add.at(cnt_hit, ends[ends >= 0], 1)
    nvis = np.zeros(len(idx), dtype=np.int64)
    gen = steps(o, d, co, s_end, res, max_steps)
    cut = np.zeros(len(idx), dtype=bool)
    try:
        while True:
            r, cells, s_in, s_out = next(gen)
            nvis[r] += 1
            cell = lookup(m, cells)
            on = cell >= 0
            on[on] = m["valid"][cell[on]] & (m["count"][cell[on]] > 0)
            r, cell, s_in, s_out = r[on], cell[on], s_in[on], s_out[on]
            through = passes(m, cell, o, d[r], s_in, s_out, sigma2)
            np.add.at(cnt_pass, cell[through], 1)
    except StopIteration as e:
        if e.value is not None:
            cut = e.value
    if visited is not None:
        visited.extend(int(v) for v in nvis)
    seen, cleared = decide(m, min_pass, miss_frames)
    return [int(len(idx)), seen, cleared, int(cut.sum())]


def decide(m, min_pass=2, miss_frames=3):
    """The decision per assigned cell from the map's ``pass`` and ``hit``: (cells seen through, cells cleared)."""
    cnt_pass, cnt_hit, miss = state(m)
    live = m["valid"] & (m["count"] > 0)
    hit = live & (cnt_hit >= 1)
    seen = live & ~hit & (cnt_pass >= min_pass)
    miss[hit] = 0
    miss[seen] += 1
    clear = live & (miss >= miss_frames)
    m["count"][clear] = 0
    m["S"][clear] = 0.0
    m["mean"][clear] = 0.0
    m["icov"][clear] = 0.0
    m["valid"][clear] = False
    miss[clear] = 0
    return int(seen.sum()), int(clear.sum())
