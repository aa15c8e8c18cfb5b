"""Numpy restatement of the NDT localiser with several hypotheses (include/sps_hip.h, "NDT localiser, several hypotheses";
DESIGN.md 8d), on top of tests/ndt_reference.py.  It shares no code with sps_amd/localiser.py and never touches the native
library: K alignments one after the other, the score and the counted points at every final pose, then the selection."""
import math
from types import SimpleNamespace

import numpy as np

from tests import localiser_reference as LR
from tests import ndt_reference as NR


def offset(a, b, yaw_deg):
    """D(a, b, psi) = [[Rz(psi), (a, b, 0)^T], [0, 1]]"""
    c, s = math.cos(math.radians(yaw_deg)), math.sin(math.radians(yaw_deg))
    return np.array([[c, 0.0 - s, 0.0, a], [s, c, 0.0, b], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def grid(along, across, yaw_deg):
    """the offsets in the order k = (ia * len(across) + ib) * len(yaw_deg) + ipsi"""
    return np.array([offset(a, b, y) for a in along for b in across for y in yaw_deg])


def select(scores, counts, statuses, min_corr):
    """the highest score among the hypotheses with status 0 or 1 and counts >= min_corr; ties to the lowest index; -1 if
    none qualifies"""
    best = -1
    for k in range(len(scores)):
        if statuses[k] in (0, 1) and counts[k] >= min_corr and (best < 0 or scores[k] > scores[best]):
            best = k
    return best


def align_batch(pts, cmap, T_inits, iters=30, neighbours=7, min_corr=50, outlier_ratio=0.55, tol_t=1e-4, tol_r=1e-5):
    """dict(results (K dicts of NR.align), scores (math.fsum of the final pose's terms), hits (NR.hits at the final
    poses: the terms behind each score), counts, best, pose)"""
    T_inits = np.asarray(T_inits, dtype=np.float64)
    results = [NR.align(pts, cmap, T, iters, neighbours, min_corr, outlier_ratio, tol_t, tol_r) for T in T_inits]
    scores, counts, hits = [], [], []
    for r in results:
        sc, h = NR.score(pts, cmap, r["pose"], neighbours, outlier_ratio)
        scores.append(sc)
        counts.append(len(np.unique(h["i"])))
        hits.append(h)
    best = select(scores, counts, [r["status"] for r in results], min_corr)
    pose = results[best]["pose"] if best >= 0 else T_inits[0].copy()
    return dict(results=results, scores=np.array(scores), counts=np.array(counts, dtype=np.int64), hits=hits, best=best, pose=pose)


class BatchLocaliser:
    """The restatement behind the interface sps_amd.localiser.LocalisationLoop uses with hypotheses
    (``submit_filtered_batch(pending, T_inits).result()`` -> an object with results, scores, counts, best, pose), so that a
    loop driven by it is the loop restated: the same filter and motion model around K numpy alignments and the selection
    above.  ``like`` supplies the settings (leaf, capacity, iterations, neighbours, ...) and the device."""

    def __init__(self, cmap, like):
        self.cmap, self.like, self.device = cmap, like, like.device

    def submit_batch(self, rows, count, T_inits):
        L = self.like
        rows = rows[:count].cpu().numpy() if hasattr(rows, "cpu") else np.asarray(rows)[:count]
        _, pts = LR.downsample(rows, int(count), L.leaf, L.capacity)
        b = align_batch(pts, self.cmap, T_inits, L.iterations, L.neighbours, L.min_correspondences, L.outlier_ratio, L.tol_t,
                        L.tol_r)
        res = SimpleNamespace(
            results=[SimpleNamespace(pose=r["pose"], status=r["status"], iterations=r["iterations"], n_corr=r["n_corr"],
                                     trace=r["trace"], n_points=len(pts)) for r in b["results"]],
            scores=b["scores"], counts=b["counts"], best=b["best"], pose=b["pose"])
        return SimpleNamespace(result=lambda: res)

    def submit_filtered_batch(self, pending, T_inits):
        return self.submit_batch(pending._filtered, int(pending.count_dev.item()), T_inits)
