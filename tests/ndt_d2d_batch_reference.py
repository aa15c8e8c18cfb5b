"""Numpy restatement of distribution-to-distribution NDT from several poses (include/sps_hip.h, "NDT localiser,
distribution to distribution, several poses").  It adds no arithmetic: the single alignment and the
per-pair terms are tests/ndt_d2d_reference.py's, the selection is tests/ndt_batch_reference.py's, the top-K rule and the
device's order of summation are tests/ndt_search_reference.py's.  It shares no code with sps_amd/localiser.py and never
touches the native library."""
import math
from types import SimpleNamespace

import numpy as np

from tests import localiser_reference as LR
from tests import ndt_batch_reference as NB
from tests import ndt_d2d_reference as DR
from tests import ndt_search_reference as NS


def select(scores, counts, statuses, min_corr):
    """ndt_batch_reference.select among the hypotheses whose score is a number: NaN never wins on the device, which takes a
    hypothesis only where its score is greater than the best so far, starting from -infinity"""
    return NB.select(scores, counts, [st if not math.isnan(sc) else -1 for sc, st in zip(scores, statuses)], min_corr)


def final_score(src, cmap, T, neighbours=7, outlier_ratio=0.55):
    """(math.fsum of the pose's score terms, sources counted, the hits behind them); a pose that is not finite scores
    (0, 0) from no hits, as the device's lookups all fail"""
    with np.errstate(all="ignore"):
        sc, h = DR.score(src, cmap, T, neighbours, outlier_ratio)
    return sc, len(np.unique(h["i"])), h


def align_batch(src, cmap, T_inits, iters=30, neighbours=7, min_corr=50, outlier_ratio=0.55, tol_t=1e-4, tol_r=1e-5, reverse=False):
    """dict(results (K dicts of DR.align), scores (math.fsum of the final pose's terms), hits (DR.hits at the final poses),
    counts (sources), best, pose): ndt_batch_reference.align_batch with the D2D alignment and score"""
    T_inits = np.asarray(T_inits, dtype=np.float64)
    results = [DR.align(src, cmap, T, iters, neighbours, min_corr, outlier_ratio, tol_t, tol_r, reverse) for T in T_inits]
    scores, counts, hits = [], [], []
    for r in results:
        sc, n, h = final_score(src, cmap, r["pose"], neighbours, outlier_ratio)
        scores.append(sc), counts.append(n), hits.append(h)
    best = select(scores, counts, [r["status"] for r in results], min_corr)
    pose = results[best]["pose"] if best >= 0 else T_inits[0].copy()
    return dict(results=results, scores=np.array(scores), counts=np.array(counts, dtype=np.int64), hits=hits, best=best, pose=pose)


def score_poses(src, cmap, poses, neighbours=7, outlier_ratio=0.55):
    """dict(scores [P] (math.fsum), ordered [P] (the same terms in the device's order: ndt_search_reference.ordered_sum
    over the source records), counts [P], m [P] (pairs of a pose), sum_abs [P], faces [P], boundary [P])"""
    out = dict(scores=[], ordered=[], counts=[], m=[], sum_abs=[], faces=[], boundary=[])
    n_rec = len(src["valid"])
    for T in np.asarray(poses, dtype=np.float64):
        sc, n, h = final_score(src, cmap, T, neighbours, outlier_ratio)
        t = h["terms"][:, 27]
        out["scores"].append(sc)
        out["ordered"].append(NS.ordered_sum(h["i"], h["c"], t, n_rec))
        out["counts"].append(n)
        out["m"].append(len(t))
        out["sum_abs"].append(math.fsum(np.abs(t)))
        out["faces"].append(h["faces"])
        out["boundary"].append(h["boundary"])
    return {k: np.array(v, dtype=np.float64 if k in ("scores", "ordered", "sum_abs") else np.int64) for k, v in out.items()}


def relocalise(src, cmap, poses, keep=8, iters=30, neighbours=7, min_corr=50, outlier_ratio=0.55, tol_t=1e-4, tol_r=1e-5):
    """dict(scores, counts, grid, candidates, n_top, starts, batch, index, pose): ndt_search_reference.relocalise with the
    D2D score and batch"""
    sc = score_poses(src, cmap, poses, neighbours, outlier_ratio)
    idx, n_top = NS.top(sc["scores"], sc["counts"], min_corr, keep)
    starts = NS.top_poses(poses, idx)
    batch = align_batch(src, cmap, starts, iters, neighbours, min_corr, outlier_ratio, tol_t, tol_r)
    index = int(idx[batch["best"]]) if batch["best"] >= 0 else -1
    return dict(scores=sc["scores"], counts=sc["counts"], grid=sc, candidates=idx, n_top=n_top, starts=starts, batch=batch,
                index=index, pose=batch["pose"])


class D2DBatchLocaliser:
    """The restatement behind the interface sps_amd.localiser.LocalisationLoop(..., d2d=True) uses with hypotheses and with
    search, so that a loop driven by it is the loop restated.  ``like`` supplies the settings and the device.  Every call
    insists on the ``d2d=True`` the loop must pass, and asserts that the frame needs neither a face nor a guard boundary."""
    source = "cells"

    def __init__(self, cmap, like):
        self.cmap, self.like, self.device = cmap, like, like.device

    def _src(self, rows, count):
        L = self.like
        rows = rows[:count].cpu().numpy() if hasattr(rows, "cpu") else np.asarray(rows)[:count]
        pts = LR.downsample(rows, int(count), L.leaf, L.capacity)[1]
        return DR.sources(pts, L.source_resolution, L.source_min_points, L.eig_ratio), len(pts)

    def _settings(self):
        L = self.like
        return L.iterations, L.neighbours, L.min_correspondences, L.outlier_ratio, L.tol_t, L.tol_r

    @staticmethod
    def _pose_result(r, n_points, n_sources):
        assert r["faces"] == 0 and r["boundary"] == 0
        return SimpleNamespace(pose=r["pose"], status=r["status"], iterations=r["iterations"], n_corr=r["n_corr"],
                               trace=r["trace"], n_points=n_points, n_sources=n_sources)

    def _batch_result(self, b, n_points, n_sources):
        return SimpleNamespace(results=[self._pose_result(r, n_points, n_sources) for r in b["results"]], scores=b["scores"],
                               counts=b["counts"], best=b["best"], pose=b["pose"])

    def submit(self, rows, count, T_init):
        src, n = self._src(rows, count)
        res = self._pose_result(DR.align(src, self.cmap, T_init, *self._settings()), n, src["n_src"][1])
        return SimpleNamespace(result=lambda: res)

    def submit_filtered(self, pending, T_init):
        return self.submit(pending._filtered, int(pending.count_dev.item()), T_init)

    def submit_batch(self, rows, count, T_inits, d2d=False):
        assert d2d is True
        src, n = self._src(rows, count)
        res = self._batch_result(align_batch(src, self.cmap, T_inits, *self._settings()), n, src["n_src"][1])
        return SimpleNamespace(result=lambda: res)

    def submit_filtered_batch(self, pending, T_inits, **kw):
        return self.submit_batch(pending._filtered, int(pending.count_dev.item()), T_inits, **kw)

    def relocalise(self, rows, count, poses, keep=8, d2d=False):
        assert d2d is True
        src, n = self._src(rows, count)
        r = relocalise(src, self.cmap, poses, keep, *self._settings())
        res = SimpleNamespace(scores=r["scores"], counts=r["counts"], candidates=r["candidates"],
                              batch=self._batch_result(r["batch"], n, src["n_src"][1]), index=r["index"], pose=r["pose"],
                              ok=r["index"] >= 0)
        return SimpleNamespace(result=lambda: res)

    def relocalise_filtered(self, pending, poses, **kw):
        return self.relocalise(pending._filtered, int(pending.count_dev.item()), poses, **kw)
