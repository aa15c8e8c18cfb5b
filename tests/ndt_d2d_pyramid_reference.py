"""Numpy restatement of distribution-to-distribution NDT registered coarse to fine (include/sps_hip.h, "NDT localiser,
distribution to distribution, pyramid"): tests/ndt_d2d_reference.py's ``sources`` once per level and its
``align`` run level after level, coarsest first, with a shared budget of slots.  It shares no code with
sps_amd/localiser.py and never touches the native library.

The handoff rule is that of tests/ndt_pyramid_reference.py with one addition.  The call starts at level 0.  Level l runs
until it converges or has used ``level_iters[l]`` slots and then hands its pose to the next level l' > l whose valid
sources (clipped to ``cap_src`` where one is given) are at least ``min_corr``; where there is none, level l is the last:
its convergence is status 0 and its cap ends the call with status 1.  Status 2 and 3 are final at any level and give the
first start pose back.  When the budget runs out the call ends with status 1 wherever it is."""
import numpy as np

from tests import ndt_d2d_reference as DR
from tests import ndt_reference as NR


def pyramid(map_xyz, resolutions, min_points=6, eig_ratio=0.01):
    """the cell maps of the levels, coarsest first"""
    return [NR.cells(map_xyz, r, min_points, eig_ratio) for r in resolutions]


def sources(pts, source_resolutions, min_points=6, eig_ratio=0.01):
    """the scan's cells of every level: ``DR.sources`` at the level's resolution and ``min_points`` (an int, or one per level)"""
    mps = [int(min_points)] * len(source_resolutions) if np.ndim(min_points) == 0 else [int(v) for v in min_points]
    assert len(mps) == len(source_resolutions)
    return [DR.sources(pts, float(r), m, eig_ratio) for r, m in zip(source_resolutions, mps)]


def valid_sources(src, cap_src=None):
    n = int(src["n_src"][1])
    return n if cap_src is None else min(n, int(cap_src))


def next_level(srcs, l, min_corr, cap_src=None):
    """the level that follows l, or -1 where l is the last: the skip rule"""
    for k in range(l + 1, len(srcs)):
        if valid_sources(srcs[k], cap_src) >= min_corr:
            return k
    return -1


def align(srcs, cmaps, T_init, iters=30, level_iters=None, neighbours=7, min_corr=50, outlier_ratio=0.55, tol_t=1e-4, tol_r=1e-5,
          reverse=False, cap_src=None):
    """dict(pose, status, iterations (slots used), n_corr and level of the last live slot, n_sources (the valid sources of
    that level), levels [slots], trace [slots, 4], normal [slots, 28], per_level (the dict DR.align returned for every level
    entered), entered (their levels), faces, boundary)."""
    L = len(cmaps)
    assert len(srcs) == L
    caps = [iters] * L if level_iters is None else [int(v) for v in level_iters]
    assert len(caps) == L and (min(caps) >= 1 or iters == 0)
    T0 = np.array(T_init, dtype=np.float64)
    T, left = T0.copy(), int(iters)
    status, n_corr, last = 1, 0, 0
    levels, trace, normal, per_level, entered, faces, boundary = [], [], [], [], [], 0, 0
    l = 0
    while l >= 0 and left > 0:
        r = DR.align(srcs[l], cmaps[l], T, min(caps[l], left), neighbours, min_corr, outlier_ratio, tol_t, tol_r, reverse)
        per_level.append(r)
        entered.append(l)
        used = r["iterations"]
        left -= used
        levels += [l] * used
        trace.append(r["trace"])
        normal.append(r["normal"])
        faces += r["faces"]
        boundary += r["boundary"]
        n_corr, last = r["n_corr"], l
        if r["status"] in (2, 3):
            status, T = r["status"], T0.copy()
            break
        T = r["pose"]
        nxt = next_level(srcs, l, min_corr, cap_src)
        if nxt < 0:
            # the last level: converged is 0; its own cap and the budget both leave 1
            status = r["status"]
        l = nxt
    return dict(pose=T, status=status, iterations=len(levels), n_corr=n_corr, level=last,
                n_sources=valid_sources(srcs[last], cap_src), levels=np.array(levels, dtype=np.int64),
                trace=np.concatenate(trace).reshape(-1, 4) if trace else np.zeros((0, 4)),
                normal=np.concatenate(normal).reshape(-1, 28) if normal else np.zeros((0, 28)), per_level=per_level,
                entered=entered, faces=faces, boundary=boundary)
