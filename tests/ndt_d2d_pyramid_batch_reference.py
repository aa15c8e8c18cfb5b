"""Numpy restatement of distribution-to-distribution NDT registered coarse to fine from several start poses
(include/sps_hip.h, "NDT localiser, distribution to distribution, pyramid, several hypotheses").  It adds no
arithmetic: K times tests/ndt_d2d_pyramid_reference.py's ``align``, the scoring level from its ``valid_sources`` /
``next_level``, every end pose scored on that level by tests/ndt_d2d_batch_reference.py's ``final_score``, then
tests/ndt_pyramid_batch_reference.py's ``select`` and ``best_words``.  It shares no code with sps_amd and never touches the
native library.

Also the scene of the tests: tests/test_hip_ndt_d2d_pyramid.py's (400 x 32 rays, the synthetic map, scan 1 thinned at leaf
0.4; map and sources at 2 / 1 / 0.5 m, min_corr = 20) with the six start poses of tests/ndt_pyramid_batch_reference.py, the
sources at three settings of min_points and four budgets, whose restated results are computed once per process."""
import functools
import math

import numpy as np

from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_d2d_batch_reference as DB
from tests import ndt_d2d_pyramid_reference as DP
from tests import ndt_pyramid_batch_reference as PB
from tests.test_ndt_cpu import KW, LEAF, sensor_scan
from tests.test_ndt_d2d_cpu import EIG_RATIO

RESOLUTIONS = (2.0, 1.0, 0.5)
MIN_CORR = 20
NAMES, POSES, OFF, WRONG = PB.NAMES, PB.POSES, PB.OFF, PB.WRONG
# source_min_points -> the levels the scan's cells walk.  3: all three; 6: the finest level has 3 valid sources and is
# skipped; (3, 1000, 1000): no cell of the scan has 1000 points, nothing qualifies beyond level 0
SOURCES = {"all": 3, "finest skipped": 6, "level 0 only": (3, 1000, 1000)}
CHAIN = {"all": [0, 1, 2], "finest skipped": [0, 1], "level 0 only": [0]}
# (caps, budget of slots): the sum of the caps; small caps; one slot each; a budget that ends in the middle of level 1
BUDGETS = (((30, 30, 30), 90), ((5, 3, 30), 38), ((1, 1, 1), 3), ((4, 30, 30), 7))


def chain(srcs, min_corr, cap_src=None):
    """the levels every hypothesis walks, in their order: level 0, then ``next_level`` until there is none"""
    out = [0]
    while True:
        nxt = DP.next_level(srcs, out[-1], min_corr, cap_src)
        if nxt < 0:
            return out
        out.append(nxt)


def scoring_level(srcs, min_corr, cap_src=None):
    """l*: the last level of the chain.  The same as the largest l >= 1 whose valid sources (clipped to cap_src) are at least
    min_corr, or 0 where there is none"""
    l = chain(srcs, min_corr, cap_src)[-1]
    direct = max([k for k in range(1, len(srcs)) if DP.valid_sources(srcs[k], cap_src) >= min_corr], default=0)
    assert l == direct
    return l


def align_batch(srcs, cmaps, T_inits, iters=30, level_iters=None, neighbours=7, min_corr=MIN_CORR, outlier_ratio=0.55,
                tol_t=1e-4, tol_r=1e-5, reverse=False, cap_src=None):
    """dict(results (K dicts of DP.align), level (l*), scores (math.fsum of the terms of every end pose with level l*'s
    sources on level l*'s map), counts (sources counted there), hits, best, pose, words (best_dev))"""
    T_inits = np.asarray(T_inits, dtype=np.float64)
    results = [DP.align(srcs, cmaps, T, iters, level_iters, neighbours, min_corr, outlier_ratio, tol_t, tol_r, reverse, cap_src)
               for T in T_inits]
    ls = scoring_level(srcs, min_corr, cap_src)
    scores, counts, hits = [], [], []
    for r in results:
        sc, n, h = DB.final_score(srcs[ls], cmaps[ls], r["pose"], neighbours, outlier_ratio)
        scores.append(sc), counts.append(n), hits.append(h)
    statuses = [r["status"] for r in results]
    best = DB.select(scores, counts, statuses, min_corr)
    pose = results[best]["pose"] if best >= 0 else T_inits[0].copy()
    return dict(results=results, level=ls, scores=np.array(scores), counts=np.array(counts, dtype=np.int64), hits=hits, best=best,
                pose=pose, words=PB.best_words(best, statuses, counts, len(T_inits)))


@functools.lru_cache(maxsize=None)
def scene():
    """dict(map_xyz, cmaps, scan (float32 rows), pts (the thinned float64 points), src (name of SOURCES -> the source cells of
    the three levels)); read-only"""
    map_xyz = synthetic.build_map(**KW)[:, :3].astype(np.float64)
    scan = sensor_scan(1)
    pts = LR.downsample(scan, len(scan), LEAF)[1]
    return dict(map_xyz=map_xyz, cmaps=DP.pyramid(map_xyz, RESOLUTIONS), scan=scan, pts=pts,
                src={name: DP.sources(pts, RESOLUTIONS, mp, EIG_RATIO) for name, mp in SOURCES.items()})


@functools.lru_cache(maxsize=None)
def restated(sources="all", budget=0, reverse=False):
    """align_batch of the six starts with the sources SOURCES[sources] at BUDGETS[budget]; read-only"""
    sc = scene()
    caps, iters = BUDGETS[budget]
    return align_batch(sc["src"][sources], sc["cmaps"], POSES, iters, caps, reverse=reverse)


def slots_per_level(levels, n_levels=len(RESOLUTIONS)):
    return [int((np.asarray(levels) == l).sum()) for l in range(n_levels)]


def check_input_properties(sources, budget, statuses, slots, levels, level=None):
    """What the tests' inputs must have for the tests to mean anything, asserted on the results of K single alignments
    (restated or on the device) of the six starts with SOURCES[sources] at BUDGETS[budget]: ``statuses`` and ``slots`` per
    start, ``levels`` the level rows (slots used), ``level`` the scoring level where the caller has one"""
    others = [k for k in range(len(NAMES)) if k != OFF]
    walk = CHAIN[sources]
    assert level is None or level == walk[-1]
    assert (statuses[OFF], slots[OFF]) == (2, 1)                               # off the map: final in its first slot ...
    assert all(slots[k] > 1 for k in others) or BUDGETS[budget][1] == 1        # ... while the others go on
    assert all(statuses[k] in (0, 1) for k in others)
    assert all(set(levels[k]) <= set(walk) for k in others)                    # nobody enters a skipped level
    if budget == 0:                                                            # the full budget: everybody ends on l*
        assert all(statuses[k] == 0 and levels[k][-1] == walk[-1] for k in others)
        if len(walk) > 1:                                                      # different levels in the same slot
            first = [PB.entered(levels[k])[walk[1]] for k in others]
            assert len(set(first)) > 1
            a, b = others[int(np.argmin(first))], others[int(np.argmax(first))]
            s = min(first)
            assert levels[a][s] != levels[b][s]
    if sources == "all" and budget == 2:                                       # one slot per level, three slots
        assert all(list(levels[k]) == [0, 1, 2] and statuses[k] == 1 for k in others)
    if sources == "all" and budget == 3:                                       # stopped before l*, yet eligible
        assert all(statuses[k] == 1 and slots[k] == 7 and levels[k][-1] == 1 and 2 not in levels[k] for k in others)
    if sources == "all" and budget == 1:                                       # small caps: a handoff forced by the cap
        assert any(slots_per_level(levels[k])[:2] == [5, 3] for k in others)


def check_scene_properties():
    """the three settings of the sources give l* = L - 1, l* < L - 1 and l* = 0"""
    sc = scene()
    got = {name: chain(srcs, MIN_CORR) for name, srcs in sc["src"].items()}
    assert got == CHAIN, got
    assert [scoring_level(sc["src"][n], MIN_CORR) for n in SOURCES] == [2, 1, 0]
    assert DP.valid_sources(sc["src"]["finest skipped"][2]) == 3               # the finest level: nobody would qualify on it
    return got


def spread_tolerance(fwd, rev):
    """this project's rule for a float64 comparison that differs only in the order of a sum: 100 x the restatement's own
    forward-versus-reversed spread, floored at 1e-12 -> (metres, radians)"""
    st, sr = LR.pose_difference(fwd, rev)
    return max(100.0 * st, 1e-12), max(100.0 * sr, 1e-12), st, sr


def score_tolerance(fwd, rev):
    """the same rule for the final score of a hypothesis, from the forward and the reversed restatement's scores"""
    return max(100.0 * abs(fwd - rev), 1e-12)
