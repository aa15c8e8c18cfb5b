"""Numpy restatement of the coarse-to-fine NDT alignment from several start poses (include/sps_hip.h, "NDT localiser, pyramid,
several hypotheses"), on top of tests/ndt_pyramid_reference.py and tests/ndt_reference.py.  It shares no code
with sps_amd/localiser.py and never touches the native library: K pyramid alignments one after the other, the score and the
counted points of every final pose on the finest level, then the selection rule, restated here.

Also the scene of the tests: test_hip_ndt_pyramid.py's (400 x 32 rays, the synthetic map, scan 1 thinned at leaf 0.4) with six
start poses and three budgets, whose restated results are computed once per process."""
import functools
import math

import numpy as np

from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_pyramid_reference as PR
from tests import ndt_reference as NR
from tests.test_ndt_cpu import KW, LEAF, T_INIT, T_TRUE, sensor_scan

RESOLUTIONS = (2.0, 1.0, 0.5)
# name -> start pose, in the order the tests use
STARTS = {
    "true": T_TRUE,
    "0.5 m along": LR.perturbation(0.5, 0.0, 0.0, 0.0) @ T_TRUE,
    "T_INIT": T_INIT,
    "1.5 m along": LR.perturbation(1.5, 0.0, 0.0, 0.0) @ T_TRUE,
    "8 deg yaw": LR.perturbation(0.0, 0.0, 0.0, 8.0) @ T_TRUE,
    "300 m off": LR.perturbation(300.0, 0.0, 0.0, 0.0) @ T_TRUE,
}
NAMES = tuple(STARTS)
POSES = np.stack([STARTS[n] for n in NAMES])
OFF = NAMES.index("300 m off")
WRONG = NAMES.index("1.5 m along")
# (caps, budget of slots)
BUDGETS = (((30, 30, 30), 90), ((4, 4, 4), 12), ((2, 2, 2), 4))


def select(scores, counts, statuses, min_corr):
    """k_ndt_select's rule: the highest score among the hypotheses with status 0 or 1 and at least min_corr points counted;
    a tie stays with the lowest index; a NaN score never wins (no comparison with it is true, not even as the first
    candidate); -1 where nobody qualifies"""
    best, top = -1, -math.inf
    for k in range(len(scores)):
        if statuses[k] in (0, 1) and counts[k] >= min_corr and scores[k] > top:
            best, top = k, scores[k]
    return best


def best_words(best, statuses, counts, n_hyp):
    """best_dev of the call: (k, its status, its count, n_hyp), or (-1, -1, 0, n_hyp)"""
    return [best, statuses[best], counts[best], n_hyp] if best >= 0 else [-1, -1, 0, n_hyp]


def align_batch(pts, cmaps, T_inits, iters=30, level_iters=None, neighbours=7, min_corr=50, outlier_ratio=0.55, tol_t=1e-4,
                tol_r=1e-5, reverse=False):
    """dict(results (K dicts of PR.align), scores (math.fsum of the terms of every final pose on the finest level), counts,
    best, pose)"""
    T_inits = np.asarray(T_inits, dtype=np.float64)
    results = [PR.align(pts, cmaps, T, iters, level_iters, neighbours, min_corr, outlier_ratio, tol_t, tol_r, reverse)
               for T in T_inits]
    scores, counts = [], []
    for r in results:
        sc, h = NR.score(pts, cmaps[-1], r["pose"], neighbours, outlier_ratio)
        scores.append(sc)
        counts.append(len(np.unique(h["i"])))
    best = select(scores, counts, [r["status"] for r in results], min_corr)
    pose = results[best]["pose"] if best >= 0 else T_inits[0].copy()
    return dict(results=results, scores=np.array(scores), counts=np.array(counts, dtype=np.int64), best=best, pose=pose)


@functools.lru_cache(maxsize=None)
def scene():
    """dict(map_xyz, cmaps, scan (float32 rows), pts (the thinned float64 points)); read-only"""
    map_xyz = synthetic.build_map(**KW)[:, :3].astype(np.float64)
    scan = sensor_scan(1)
    _, pts = LR.downsample(scan, len(scan), LEAF)
    return dict(map_xyz=map_xyz, cmaps=PR.pyramid(map_xyz, RESOLUTIONS), scan=scan, pts=pts)


@functools.lru_cache(maxsize=None)
def restated(budget, reverse=False):
    """align_batch of the six starts at BUDGETS[budget]; read-only"""
    sc = scene()
    caps, iters = BUDGETS[budget]
    return align_batch(sc["pts"], sc["cmaps"], POSES, iters, caps, reverse=reverse)


def entered(levels):
    """the slot at which a hypothesis first stood at each level it reached: {level: slot}"""
    return {int(l): int(np.argmax(np.asarray(levels) == l)) for l in np.unique(levels)}


def check_input_properties(budget, statuses, slots, levels, poses=None, scores=None):
    """What the tests' inputs must have for the tests to mean anything, asserted on the results of K single alignments
    (restated or on the device) of the six starts at BUDGETS[budget]: ``statuses`` and ``slots`` per start, ``levels`` the level
    rows (slots used); with the full budget also ``poses`` and the finest-level ``scores``"""
    others = [k for k in range(len(NAMES)) if k != OFF]
    assert (statuses[OFF], slots[OFF]) == (2, 1)                               # off the map: final in its first slot
    if budget == 0:
        assert [statuses[k] for k in others] == [0] * 5
        assert [slots[k] for k in others] == [23, 34, 28, 90, 29]
        first = [entered(levels[k]) for k in others]
        assert all(set(f) == {0, 1, 2} for f in first)
        assert first[0][1] == 7 and first[1][1] == 18                          # different levels in the same slot
        if poses is not None:
            err = [LR.pose_difference(poses[k], T_TRUE)[0] for k in range(len(NAMES))]
            assert 0.8 < err[WRONG] < 1.0 and all(err[k] < 0.02 for k in others if k != WRONG)   # the wrong basin, status 0
        if scores is not None:
            assert abs(scores[0] - 1583.93) < 0.01 and scores[WRONG] < scores[0] - 1.0
    elif budget == 1:
        assert [statuses[k] for k in others] == [1] * 5 and [slots[k] for k in others] == [12] * 5
        assert all(levels[k][-1] == 2 for k in others)
    else:
        assert [statuses[k] for k in others] == [1] * 5 and [slots[k] for k in others] == [4] * 5
        assert all(levels[k][-1] == 1 and 2 not in levels[k] for k in others)  # stopped before the finest level, yet eligible
