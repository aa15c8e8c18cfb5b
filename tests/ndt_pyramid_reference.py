"""Numpy restatement of the multi-resolution NDT alignment (include/sps_hip.h, "NDT localiser, multi-resolution pyramid";
DESIGN.md 8g): tests/ndt_reference.py's ``align`` run level after level, coarsest first, with a shared budget of slots.
It shares no code with sps_amd/localiser.py and never touches the native library.

The handoff rule: level l runs until it converges or has used ``level_iters[l]`` slots, whichever comes first, and then hands
its pose to level l + 1; only the last level's convergence is status 0.  Status 2 and 3 are final at any level and give the
first start pose back.  When the budget runs out the call ends with status 1 wherever it is."""
import numpy as np

from tests import ndt_reference as NR


def pyramid(map_xyz, resolutions, min_points=6, eig_ratio=0.01):
    """the cell maps of the levels, coarsest first"""
    return [NR.cells(map_xyz, r, min_points, eig_ratio) for r in resolutions]


def align(pts, cmaps, T_init, iters=30, level_iters=None, neighbours=7, min_corr=50, outlier_ratio=0.55, tol_t=1e-4, tol_r=1e-5,
          reverse=False):
    """dict(pose, status, iterations (slots used), n_corr and level of the last live slot, levels [slots], trace [slots, 4],
    normal [slots, 28], per_level (the dict NR.align returned for every level entered), faces, boundary)."""
    L = len(cmaps)
    caps = [iters] * L if level_iters is None else [int(v) for v in level_iters]
    assert len(caps) == L and (min(caps) >= 1 or iters == 0)
    T0 = np.array(T_init, dtype=np.float64)
    T, left = T0.copy(), int(iters)
    status, n_corr, last = 1, 0, 0
    levels, trace, normal, per_level, faces, boundary = [], [], [], [], 0, 0
    for l in range(L):
        if left == 0:
            break
        r = NR.align(pts, cmaps[l], T, min(caps[l], left), neighbours, min_corr, outlier_ratio, tol_t, tol_r, reverse)
        per_level.append(r)
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
        if l == L - 1:
            status = r["status"]
    return dict(pose=T, status=status, iterations=len(levels), n_corr=n_corr, level=last, levels=np.array(levels, dtype=np.int64),
                trace=np.concatenate(trace).reshape(-1, 4) if trace else np.zeros((0, 4)),
                normal=np.concatenate(normal).reshape(-1, 28) if normal else np.zeros((0, 28)), per_level=per_level,
                faces=faces, boundary=boundary)
