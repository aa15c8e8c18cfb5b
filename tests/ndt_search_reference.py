"""Numpy restatement of the NDT pose search (include/sps_hip.h, "NDT localiser, pose search"), on top of
tests/ndt_reference.py and tests/ndt_batch_reference.py.  It shares no code with sps_amd/localiser.py and never touches
the native library: the score and the count of a pose (math.fsum, and once more in the kernels' order of summation), the
top-K rule, and relocalise = score, top-K, ndt_batch_reference.align_batch from the K poses."""
import math
from types import SimpleNamespace

import numpy as np

from tests import localiser_reference as LR
from tests import ndt_batch_reference as NB
from tests import ndt_reference as NR

PTS, SEG = 32, 8               # LOC_PTS, LOC_SEG: points of a workgroup, runs of consecutive workgroups


def ordered_sum(i, c, values, n):
    """values of the contributing (point i, lookup position c) pairs added as the device adds them: the cells of a point in
    lookup order, the PTS points of a block in point order, the blocks as SEG runs of consecutive blocks, then the runs."""
    term = np.zeros(max(-(-n // PTS), 1) * PTS)
    for pos in range(7):
        on = c == pos
        term[i[on]] = term[i[on]] + values[on]
    blocks = term.reshape(-1, PTS)
    rows = -(-n // PTS)
    part = np.zeros(len(blocks))
    for p in range(PTS):
        part = part + blocks[:, p]
    per = -(-rows // SEG)
    total = 0.0
    for sg in range(SEG):
        s = 0.0
        for b in range(sg * per, min(rows, (sg + 1) * per)):
            s = s + part[b]
        total = total + s
    return float(total)


def score_poses(pts, cmap, poses, neighbours=7, outlier_ratio=0.55):
    """dict(scores [P] (math.fsum of the pose's terms: ndt_batch_reference's final score), ordered [P] (the same terms in
    the device's order), counts [P], m [P] (terms of a pose), sum_abs [P], faces [P])"""
    d1, d2 = NR.gauss(outlier_ratio, cmap["resolution"])
    out = dict(scores=[], ordered=[], counts=[], m=[], sum_abs=[], faces=[])
    for T in np.asarray(poses, dtype=np.float64):
        with np.errstate(invalid="ignore"):
            h = NR.hits(LR.transform(pts, T), cmap, neighbours, d1, d2)
        t = h["terms"][:, 27]
        out["scores"].append(math.fsum(t))
        out["ordered"].append(ordered_sum(h["i"], h["c"], t, len(pts)))
        out["counts"].append(len(np.unique(h["i"])))
        out["m"].append(len(t))
        out["sum_abs"].append(math.fsum(np.abs(t)))
        out["faces"].append(h["faces"])
    return {k: np.array(v, dtype=np.float64 if k in ("scores", "ordered", "sum_abs") else np.int64) for k, v in out.items()}


def sum_bound(m, n_points, sum_abs):
    """the device's score against math.fsum: m terms and ceil(n / 32) block sums added one by one, plus 40 for the terms'
    own roundings"""
    return (m + -(-n_points // PTS) + 40) * 2.0 ** -52 * sum_abs


def top(scores, counts, min_corr, k):
    """(indices [k], n_top): the poses with counts >= min_corr and a score that is not NaN by (score descending, index
    ascending); the slots past them hold -1"""
    q = [p for p in range(len(scores)) if counts[p] >= min_corr and not math.isnan(scores[p])]
    q.sort(key=lambda p: (-scores[p], p))
    idx = q[:k] + [-1] * (k - len(q[:k]))
    return np.array(idx, dtype=np.int64), len(q[:k])


def top_poses(poses, idx):
    """[k, 4, 4]: the pose of every slot; an unfilled slot holds the pose of slot 0, or poses[0] where no slot is filled"""
    poses = np.asarray(poses, dtype=np.float64)
    fill = poses[idx[0]] if idx[0] >= 0 else poses[0]
    return np.stack([poses[i] if i >= 0 else fill for i in idx])


def relocalise(pts, cmap, poses, keep=8, iters=30, neighbours=7, min_corr=50, outlier_ratio=0.55, tol_t=1e-4, tol_r=1e-5,
               scores=None):
    """dict(scores, counts, grid (the whole score_poses dict), candidates, n_top, starts, batch (NB.align_batch), index, pose)"""
    sc = scores if scores is not None else score_poses(pts, cmap, poses, neighbours, outlier_ratio)
    idx, n_top = top(sc["scores"], sc["counts"], min_corr, keep)
    starts = top_poses(poses, idx)
    batch = NB.align_batch(pts, cmap, starts, iters, neighbours, min_corr, outlier_ratio, tol_t, tol_r)
    index = int(idx[batch["best"]]) if batch["best"] >= 0 else -1
    return dict(scores=sc["scores"], counts=sc["counts"], grid=sc, candidates=idx, n_top=n_top, starts=starts, batch=batch,
                index=index, pose=batch["pose"])


class SearchLocaliser(NB.BatchLocaliser):
    """The restatement behind the interface sps_amd.localiser.LocalisationLoop uses with ``search``: ``submit`` /
    ``submit_filtered`` (one numpy alignment) and ``relocalise`` / ``relocalise_filtered``.  ``like`` supplies the settings."""

    def _pts(self, rows, count):
        rows = rows[:count].cpu().numpy() if hasattr(rows, "cpu") else np.asarray(rows)[:count]
        return LR.downsample(rows, int(count), self.like.leaf, self.like.capacity)[1]

    @staticmethod
    def _pose_result(r, n_points):
        return SimpleNamespace(pose=r["pose"], status=r["status"], iterations=r["iterations"], n_corr=r["n_corr"],
                               trace=r["trace"], n_points=n_points)

    def submit(self, rows, count, T_init):
        L = self.like
        pts = self._pts(rows, count)
        r = NR.align(pts, self.cmap, T_init, L.iterations, L.neighbours, L.min_correspondences, L.outlier_ratio, L.tol_t, L.tol_r)
        res = self._pose_result(r, len(pts))
        return SimpleNamespace(result=lambda: res)

    def submit_filtered(self, pending, T_init):
        return self.submit(pending._filtered, int(pending.count_dev.item()), T_init)

    def relocalise(self, rows, count, poses, keep=8):
        L = self.like
        pts = self._pts(rows, count)
        r = relocalise(pts, self.cmap, poses, keep, L.iterations, L.neighbours, L.min_correspondences, L.outlier_ratio, L.tol_t,
                       L.tol_r)
        b = r["batch"]
        batch = SimpleNamespace(results=[self._pose_result(x, len(pts)) for x in b["results"]], scores=b["scores"],
                                counts=b["counts"], best=b["best"], pose=b["pose"])
        res = SimpleNamespace(scores=r["scores"], counts=r["counts"], candidates=r["candidates"], batch=batch, index=r["index"],
                              pose=r["pose"], ok=r["index"] >= 0)
        return SimpleNamespace(result=lambda: res)

    def relocalise_filtered(self, pending, poses, keep=8):
        return self.relocalise(pending._filtered, int(pending.count_dev.item()), poses, keep)
