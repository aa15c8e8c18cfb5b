"""Scan-to-map localiser and the closed loop around a scan filter.

In the reference's localisation experiment (c_ws/src/sps_filter/scripts/exp_pipeline/loc_exp_general.bash) the chosen
filter publishes a filtered cloud, hdl_localization (an external package) registers it against the map, and the
corrected pose goes back into the filter (sps_node.py reads it as odometry, sps_node_cvm.py:112-114 appends it to the
constant-velocity pose list) and is recorded for evo_ape.

``ScanToMapLocaliser`` plays the role of that package.  It is NOT a port of it -- no NDT, no UKF, no IMU -- but a
deterministic point-to-point ICP on the device (C ABI: the "localiser" section of include/sps_hip.h; DESIGN.md
"Localiser"): voxel-grid thinning of the kept rows, then ``iterations`` rounds of nearest-neighbour association within
``max_distance`` (ties to the lowest map index) and a 6 x 6 Gauss-Newton step, all in float64 with fixed-order sums, so
the same input gives the same bits.  ``submit()`` issues everything on the caller's current stream and never
synchronises; ``PendingPose.result()`` is the one synchronisation.  A scan that misses the map is an ordinary result
(status 2), never an error.

``NDTLocaliser`` is the same stage with the registration the experiment actually runs: a normal-distributions
transform (ndt_omp's 1 m cells and DIRECT7 neighbourhood by default; C ABI: the "NDT localiser" section; DESIGN.md
"NDT localiser").  Thinning, the 6 x 6 solve, the outputs and the status codes are the ICP's.  The package's other two
parts, the UKF and its IMU prediction, are ``sps_amd.pose_estimator.PoseEstimator``, which
``LocalisationLoop(..., estimator=...)`` puts around either localiser.

``NDTLocaliser.submit_batch`` registers one scan from several start poses in the same launches and selects among the
end poses by the NDT score at each (C ABI: "NDT localiser, several hypotheses"): a start in the wrong basin
converges there with status 0, and only the score tells.  ``pose_grid`` builds the offsets.

``NDTLocaliser.score_poses`` gives the NDT score of up to 65536 poses, and ``NDTLocaliser.relocalise`` scores such a grid,
keeps the best ``keep`` <= 64 on the device and registers from those (C ABI: "NDT localiser, pose search"):
for a pose known to a few metres and a few tens of degrees only.

``NDTLocaliser(..., cell_capacity=N)`` keeps an online map (C ABI: "NDT localiser, online map"): per-cell
moments for up to N cells, and ``integrate`` / ``submit(..., integrate=True)`` fold a frame's thinned points into them at
a host pose or at the frame's own corrected pose, on the frame's stream and gated by its status on the device.
``carve`` / ``submit(..., carve=True)`` do the opposite for what left the scene (C ABI: "NDT localiser, online map: free-space
carving"): the frame's points are the ends of rays from the sensor, and a cell whose Gaussian such rays pass
through for ``miss_frames`` frames on end while none ends in it is cleared.

``NDTLocaliser(..., resolutions=(2.0, 1.0, 0.5))`` registers coarse to fine (C ABI: "NDT localiser, multi-resolution
pyramid"): one static map per resolution beside the single one, and ``submit`` / ``submit_filtered`` /
``__call__`` run one alignment that starts on the coarsest map and hands its pose to the next finer one on the device.

``submit_batch``, ``submit_from_device`` and ``relocalise`` take ``coarse_to_fine=True`` on such a localiser (C ABI: "NDT
localiser, pyramid, several hypotheses"): their hypotheses are then registered on the pyramid, each at a level
of its own, from start poses that live on the device, and selected by the score on the finest level.  With
``d2d_pyramid=True`` on a localiser with ``source="cells"`` and ``source_resolutions`` they register the scan's cells on the
pyramid instead (C ABI: "NDT localiser, distribution to distribution, pyramid, several hypotheses"), selected by
the score on the last level the scan's cells do not skip.

``NDTLocaliser(..., resolutions=(2.0, 1.0, 0.5), level_capacities=(c0, c1, c2))`` makes that pyramid an online one (C ABI:
"NDT localiser, online pyramid"): every level is a dynamic map, and ``integrate`` / ``carve`` / ``submit(...,
integrate=True, carve=True)`` update and carve all levels in one set of launches; their results are then tuples, one entry per
level, coarsest first.  The single map at ``resolution`` stays static.

``NDTLocaliser(..., global_grid=dict(resolution=0.5, map_z=(lo, hi), levels=3))`` can find a pose with no start pose (C ABI:
"NDT localiser, global search"): a height slice of the map becomes a pyramid of 2-D occupancy grids, and
``global_search`` scores every cell and heading by the scan points that fall on occupied cells, level by level within a
frontier, and says how many of its best leaves are provably the exhaustive search's; ``localise_global`` hands those leaves
to the batched registration on the device.

Either localiser takes ``match_status=dict(...)`` (C ABI: "localiser, scan-matching status"): the share of the
scan's points with a map point nearby at the pose handed on, and their mean squared distance, follow every registration on
the device, and their verdict closes the gates of the map update, the carve and the estimator on a registration that
converged to the wrong place; ``LocalisationLoop(..., recover=...)`` answers such frames through the global search.

``LocalisationLoop`` closes the loop for any of the seven filters of scripts/filter_sequence.py, around either localiser.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _native
from .baseline_filters import _device_of, _pose

CONVERGED, EXHAUSTED, FEW_CORRESPONDENCES, SINGULAR = 0, 1, 2, 3
LOST = 4                       # SPS_LOC_LOST: a verdict of the scan-matching status, never a registration's status
STATUS_NAMES = {CONVERGED: "converged", EXHAUSTED: "iterations exhausted", FEW_CORRESPONDENCES: "too few correspondences",
                SINGULAR: "singular system", LOST: "lost: the scan does not match the map at the pose"}

MATCH_DEFAULTS = dict(max_distance=0.5, max_range=None, min_inlier_fraction=0.0, max_error=math.inf, min_valid=1)
MATCH_WORDS = 6                # doubles of a status: (inlier_fraction, matching_error, sum_d2, 0) | int32 (verdict, n_valid, n_inliers, n)


@dataclass
class MatchStatus:
    inlier_fraction: float     # n_inliers / max(n_valid, 1)
    matching_error: float      # the inliers' mean squared distance to their nearest map point (inf without inliers)
    n_valid: int               # thinned points that are finite and within max_range
    n_inliers: int             # of those, the points with a map point within max_distance
    verdict: int               # the registration's gate word where it had failed (2, 3, -1); else that word, or LOST
    lost: bool                 # verdict == LOST


def _match_of(words) -> MatchStatus:
    """the MatchStatus of the MATCH_WORDS float64 words the device wrote"""
    verdict, n_valid, n_in, _ = (int(x) for x in words[4:6].view(np.int32))
    return MatchStatus(float(words[0]), float(words[1]), n_valid, n_in, verdict, verdict == LOST)


def _checked_match(match_status):
    """None, or the options of the scan-matching status with the defaults filled in, before any device work"""
    if match_status is None:
        return None
    unknown = set(match_status) - set(MATCH_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown match_status entries {sorted(unknown)}")
    m = dict(MATCH_DEFAULTS, **match_status)
    try:
        m["max_distance"], m["min_inlier_fraction"], m["max_error"] = (float(m[k]) for k in ("max_distance", "min_inlier_fraction",
                                                                                            "max_error"))
        m["max_range"] = None if m["max_range"] is None else float(m["max_range"])
        if m["min_valid"] != int(m["min_valid"]):
            raise ValueError
        m["min_valid"] = int(m["min_valid"])
    except (TypeError, ValueError):
        raise ValueError("match_status: max_distance, max_range, min_inlier_fraction and max_error must be numbers and "
                         "min_valid an integer") from None
    if not (math.isfinite(m["max_distance"]) and m["max_distance"] > 0):
        raise ValueError("match_status: max_distance must be finite and > 0")
    if m["max_range"] is not None and not m["max_range"] >= 0:
        raise ValueError("match_status: max_range must be None or >= 0")
    if not 0.0 <= m["min_inlier_fraction"] <= 1.0 or not m["max_error"] >= 0 or m["min_valid"] < 0:
        raise ValueError("match_status: min_inlier_fraction must be in [0, 1], max_error >= 0 and min_valid >= 0")
    return m


@dataclass
class PoseResult:
    pose: np.ndarray           # 4x4 float64; the initial guess, bit for bit, on status 2 and 3
    status: int                # 0 converged, 1 iterations exhausted, 2 too few correspondences, 3 singular system
    iterations: int            # iterations run
    n_corr: int                # correspondences of the last iteration run
    rmse: float                # sqrt(sum d^2 / n_corr) of the last iteration run, before its update (NaN without one)
    trace: np.ndarray          # [iterations, 4] (n_corr, sum d^2, |v|, |omega|) per iteration run
    normal: np.ndarray = None  # [iterations, 28] H (upper triangle), b, sum d^2 -- only with with_normal=True
    n_points: int = 0          # scan points that entered the alignment (after thinning)
    map_update: object = None  # MapUpdateResult of the frame, with integrate=True (an online pyramid: a tuple, one per level)
    levels: np.ndarray = None  # [iterations] int, the pyramid level every slot ran at (None without a pyramid)
    map_carve: object = None   # MapCarveResult of the frame, with carve=True (an online pyramid: a tuple, one per level)
    n_sources: int = 0         # valid source cells of the scan (NDTLocaliser(source="cells") only; n_corr then counts sources)
    # MatchStatus at ``pose``, of a localiser with match_status (None without): set by ``result()``, not a field, so the
    # fields and their positional order stay what they were
    match = None

    @property
    def ok(self) -> bool:
        return self.status in (CONVERGED, EXHAUSTED)


@dataclass
class MapUpdateResult:
    cells: int                 # cells assigned after the update
    founded: int               # cells founded by this update
    dropped: int               # cells this update could not found for lack of capacity (their points were dropped)
    points: int                # points integrated; 0 with founded = dropped = 0 also where the gate was closed
    n_points: int = 0          # points that were offered (after thinning)


def _map_update_of(words, n_points) -> MapUpdateResult:
    return MapUpdateResult(int(words[0]), int(words[1]), int(words[2]), int(words[3]), int(n_points))


@dataclass
class MapCarveResult:
    rays: int                  # rays cast: the offered points whose end and origin have a cell; 0 where the gate was closed
    seen_through: int          # valid cells that rays passed through (>= min_pass of them) while none ended there
    cleared: int               # cells cleared by this carve (seen through miss_frames times on end)
    cut: int                   # rays stopped at max_steps cells before they reached their end margin
    n_points: int = 0          # points that were offered (after thinning)


def _map_carve_of(words, n_points) -> MapCarveResult:
    return MapCarveResult(int(words[0]), int(words[1]), int(words[2]), int(words[3]), int(n_points))


def _per_level(make, words, n_points, n_levels):
    """one result from four info words (n_levels None), or a tuple of them from int32[n_levels][4], coarsest first"""
    if n_levels is None:
        return make(words[:4], n_points)
    return tuple(make(words[4 * l:4 * l + 4], n_points) for l in range(n_levels))


CARVE_DEFAULTS = dict(end_margin=None, through_sigma=1.0, min_pass=2, miss_frames=3, max_steps=512)
MAX_CARVE_STEPS = 4096


def _offsets(parts, tail=()):
    """offsets (in the words of the buffer) of the named parts of one device buffer, in their order: ``size`` is where
    ``parts`` end and ``tail`` begins (a part of no words still has its offset), ``total`` where the buffer ends"""
    o, at = {}, 0
    for name, size in parts:
        o[name] = at
        at += size
    o["size"] = at
    for name, size in tail:
        o[name] = at
        at += size
    o["total"] = at
    return o


def _pose_layout(K, with_normal, pyramid=False, L=None, integrate=False, carve=False, match=False, sources=0):
    """offsets (in doubles) of a frame's one float64 buffer: T_out[16] | status int32[4] | n_points int32 (+ n_sources int32
    in the pad) | trace[K][4] | normal[K][28] | valid sources int32[sources] (+ pad), one per level of a pyramid of source
    cells | level int32[K] (+ pad) with a pyramid | info int32[4] of the update | info
    int32[4] of the carve (an online pyramid of L levels: int32[L][4] each) | the MATCH_WORDS words of the scan-matching
    status, last, with ``match``.  ``hands_on``: the offsets in bytes of the pose the frame hands on and of the int32 that
    gates what follows it on the device: ``T_out`` and the status or, with ``match``, the status' verdict"""
    w = 2 if L is None else 2 * L                                    # doubles of one call's info words
    o = _offsets((("T_out", 16), ("status", 2), ("n_points", 1), ("trace", 4 * K), ("normal", 28 * K if with_normal else 0)),
                 (("sources", (sources + 1) // 2), ("levels", (K + 1) // 2 if pyramid else 0), ("update", w if integrate else 0),
                  ("carve", w if carve else 0), ("match", MATCH_WORDS if match else 0)))
    o["hands_on"] = (o["T_out"] * 8, (o["match"] + 4) * 8 if match else o["status"] * 8)
    return o


def _batch_layout(K, I, with_normal, integrate=False, carve=False, pyramid=False, L=None, match=False, sources=0):
    """offsets (in doubles) of a batch's one float64 buffer: T_out[K][16] | status int32[K][4] | n_points int32 (+ n_sources
    int32 of a d2d batch in the pad) |
    best int32[4] | T_best[16] | final[K][2] | trace[K][I][4] | normal[K][I][28] | valid sources int32[sources] (+ pad), one
    per level, of a batch on a pyramid of source cells (``sources``: 0, or ``(levels, capacity, min_correspondences)``,
    from which the host tells the scoring level) | level int32[K][I] (+ pad) of a coarse-to-fine
    batch (``pyramid``) | info int32[4] of the update | info int32[4] of the carve (an online pyramid of L levels: int32[L][4]
    each) | the MATCH_WORDS words of the scan-matching status with ``match``.  ``hands_on``, as in ``_pose_layout``:
    ``T_best`` and ``best[1]``, the selected hypothesis' status, -1 where none was selected, or, with ``match``, the verdict"""
    w = 2 if L is None else 2 * L                                    # doubles of one call's info words
    o = _offsets((("T_out", 16 * K), ("status", 2 * K), ("n_points", 1), ("best", 2), ("T_best", 16), ("final", 2 * K),
                  ("trace", 4 * K * I), ("normal", 28 * K * I if with_normal else 0)),
                 (("sources", (_source_levels(sources) + 1) // 2), ("levels", (K * I + 1) // 2 if pyramid else 0),
                  ("update", w if integrate else 0), ("carve", w if carve else 0), ("match", MATCH_WORDS if match else 0)))
    o["hands_on"] = (o["T_best"] * 8, (o["match"] + 4) * 8 if match else o["best"] * 8 + 4)
    return o


def _source_levels(sources) -> int:
    """the levels of a pyramid of source cells from the ``sources`` of ``_batch_layout``: 0 (no such pyramid), or the first
    of ``(levels, capacity, min_correspondences)``"""
    if not sources:
        return 0
    levels, _, _ = sources                                           # nothing but the triple: ``_parse`` needs all of it
    return int(levels)


def _scoring_level(valid, capacity, min_corr) -> int:
    """the level a batch on a pyramid of source cells takes its final scores on, from the levels' valid source cells: the
    last level that is not skipped, the largest l >= 1 with min(capacity, valid[l]) >= min_corr, or 0"""
    best = 0
    for l in range(1, len(valid)):
        if min(int(capacity), max(int(valid[l]), 0)) >= int(min_corr):
            best = l
    return best


def _map_op_layout(L=None):
    """offsets (in int32 words) of the one int32 buffer of ``integrate`` / ``carve``: n_points (+ pad) | info[4] (an online
    pyramid of L levels: [L][4])"""
    return _offsets((("n_points", 4), ("info", 4 * (L or 1))))


class _Pending:
    """Work that has been issued: the pinned host copy of its one device buffer, the event behind that copy, and ``keep``,
    the tensors the work reads and writes (rows, count, the device buffer, then the poses on the host and the device)."""

    def __init__(self, host, event, keep):
        self._host, self._event, self._keep = host, event, keep

    def _wait(self) -> np.ndarray:
        self._event.synchronize()                                    # the one host synchronisation
        return self._host.numpy()

    def _pose_on_device(self):
        """(the device buffer, the address in it of the pose the work hands on, the address of that pose's gate), for what
        is queued behind the work: a registration's ``_layout()`` tells, from double ``_at`` of the buffer on"""
        out = self._keep[2]
        return (out,) + tuple(out.data_ptr() + self._at * 8 + b for b in self._layout()["hands_on"])


class _PendingMapOp(_Pending):
    _make = None                                                     # the result of four info words

    def __init__(self, host, event, keep, n_levels=None):
        super().__init__(host, event, keep)
        self._n_levels = n_levels

    def result(self):
        h, o = self._wait(), _map_op_layout(self._n_levels)
        return _per_level(self._make, h[o["info"]:], h[o["n_points"]], self._n_levels)


class PendingMapCarve(_PendingMapOp):
    """A carve whose work has been issued; ``result()`` -> MapCarveResult (an online pyramid: a tuple, one per level)."""
    _make = staticmethod(_map_carve_of)


class PendingMapUpdate(_PendingMapOp):
    """A map update whose work has been issued; ``result()`` -> MapUpdateResult (an online pyramid: a tuple, one per level)."""
    _make = staticmethod(_map_update_of)


class PendingPose(_Pending):
    """A localisation whose work has been issued; everything lives on the device until result()."""
    _at = 0

    def __init__(self, iters, with_normal, host, event, keep, pyramid=False, n_levels=None, integrate=False, carve=False,
                 match=False, sources=0):
        super().__init__(host, event, keep)
        self._sources = sources                                      # levels of a pyramid of source cells (0: none)
        self._iters, self._with_normal, self._pyramid = iters, with_normal, pyramid
        self._n_levels = n_levels                                    # an online pyramid: info words per level, tuples out
        self._integrate, self._carve = integrate, carve              # the frame's buffer has their info words
        self._match = match                                          # and those of the scan-matching status

    def _layout(self):
        return _pose_layout(self._iters, self._with_normal, self._pyramid, self._n_levels, self._integrate, self._carve,
                            self._match, self._sources)

    def result(self) -> PoseResult:
        h, o = self._wait(), self._layout()
        K, L = self._iters, self._n_levels
        code, it, n_corr, last_level = (int(x) for x in h[o["status"]:o["n_points"]].view(np.int32))
        n_points, n_sources = (int(x) for x in h[o["n_points"]:o["trace"]].view(np.int32))
        if self._sources:                                            # the level of the last live slot tells whose count
            n_sources = int(h[o["sources"]:o["levels"]].view(np.int32)[min(max(last_level, 0), self._sources - 1)])
        trace = h[o["trace"]:o["normal"]].reshape(K, 4)[:it].copy()
        normal = h[o["normal"]:o["size"]].reshape(K, 28)[:it].copy() if self._with_normal else None
        rmse = math.sqrt(trace[-1, 1] / n_corr) if it and n_corr > 0 else float("nan")
        levels = h[o["levels"]:o["update"]].view(np.int32)[:it].astype(np.int64) if self._pyramid else None
        upd = _per_level(_map_update_of, h[o["update"]:o["carve"]].view(np.int32), n_points, L) if self._integrate else None
        carved = _per_level(_map_carve_of, h[o["carve"]:o["match"]].view(np.int32), n_points, L) if self._carve else None
        res = PoseResult(h[o["T_out"]:o["status"]].reshape(4, 4).copy(), code, it, n_corr, rmse, trace, normal, n_points, upd,
                         levels, carved, n_sources)
        if self._match:
            res.match = _match_of(h[o["match"]:o["total"]])
        return res


@dataclass
class BatchPoseResult:
    results: list              # K PoseResult, hypothesis k as a single alignment from its start pose would give it
    scores: np.ndarray         # [K] the NDT score at the final pose of every hypothesis
    counts: np.ndarray         # [K] int, the scan points counted at that pose
    best: int                  # the hypothesis selected, or -1 where none has status 0 / 1 and enough points counted
    pose: np.ndarray           # 4x4: results[best].pose, or the first start pose when best is -1
    map_update: object = None  # MapUpdateResult of the frame, with integrate=True (an online pyramid: a tuple, one per level)
    map_carve: object = None   # MapCarveResult of the frame, with carve=True (an online pyramid: a tuple, one per level)
    match: object = None       # MatchStatus at ``pose``, of a localiser with match_status (None without)
    n_sources: int = None      # d2d_pyramid: the valid source cells of the level the final scores were taken on
    score_level: int = None    # d2d_pyramid: that level


class PendingPoses(_Pending):
    """A batch of localisations whose work has been issued; everything lives on the device until result()."""

    def __init__(self, n_hyp, iters, with_normal, host, event, keep, at=0, integrate=False, carve=False, pyramid=False,
                 n_levels=None, match=False, sources=0):
        super().__init__(host, event, keep)
        self._sources = sources                                      # a pyramid of source cells: (levels, capacity, min_corr)
        self._match = match                                          # the batch's buffer has the scan-matching status
        self._n_hyp, self._iters, self._with_normal = n_hyp, iters, with_normal
        self._at = at                                                # doubles in front of the batch's part of the buffer
        self._integrate, self._carve = integrate, carve              # the batch's buffer has their info words
        self._pyramid, self._n_levels = pyramid, n_levels            # coarse to fine: level rows; online: info words per level

    def _layout(self):
        return _batch_layout(self._n_hyp, self._iters, self._with_normal, self._integrate, self._carve, self._pyramid,
                             self._n_levels, self._match, self._sources)

    def result(self) -> BatchPoseResult:
        return self._parse(self._wait())

    def _parse(self, host) -> BatchPoseResult:
        h, o = host[self._at:], self._layout()
        K, I = self._n_hyp, self._iters
        T_out = h[o["T_out"]:o["status"]].reshape(K, 4, 4)
        status = h[o["status"]:o["n_points"]].view(np.int32).reshape(K, 4)
        n_points, n_sources = (int(x) for x in h[o["n_points"]:o["best"]].view(np.int32))   # sources: a d2d batch only
        best = h[o["best"]:o["T_best"]].view(np.int32)
        final = h[o["final"]:o["trace"]].reshape(K, 2)
        trace = h[o["trace"]:o["normal"]].reshape(K, I, 4)
        normal = h[o["normal"]:o["size"]].reshape(K, I, 28) if self._with_normal else None
        levels = h[o["levels"]:o["update"]].view(np.int32)[:K * I].reshape(K, I) if self._pyramid else None
        valid = h[o["sources"]:o["levels"]].view(np.int32)[:_source_levels(self._sources)] if self._sources else None
        results = []
        for k in range(K):
            code, it, n_corr, last_level = (int(x) for x in status[k])
            if valid is not None:                                    # as ``submit``: the level of the last live slot tells
                n_sources = int(valid[min(max(last_level, 0), len(valid) - 1)])
            tr = trace[k, :it].copy()
            rmse = math.sqrt(tr[-1, 1] / n_corr) if it and n_corr > 0 else float("nan")
            results.append(PoseResult(T_out[k].copy(), code, it, n_corr, rmse, tr,
                                      normal[k, :it].copy() if normal is not None else None, n_points,
                                      levels=levels[k, :it].astype(np.int64) if levels is not None else None,
                                      n_sources=n_sources))
        L = self._n_levels
        upd = _per_level(_map_update_of, h[o["update"]:o["carve"]].view(np.int32), n_points, L) if self._integrate else None
        carved = _per_level(_map_carve_of, h[o["carve"]:o["match"]].view(np.int32), n_points, L) if self._carve else None
        match = _match_of(h[o["match"]:o["total"]]) if self._match else None
        out = BatchPoseResult(results, final[:, 0].copy(), final[:, 1].astype(np.int64), int(best[0]),
                              h[o["T_best"]:o["final"]].reshape(4, 4).copy(), upd, carved, match)
        if valid is not None:
            out.score_level = _scoring_level(valid, *self._sources[1:])
            out.n_sources = int(valid[out.score_level])
        return out


def pose_grid(along, across, yaw_deg) -> np.ndarray:
    """Body-frame offsets D(a, b, psi) = [[Rz(psi), (a, b, 0)^T], [0, 1]] as float64 [K, 4, 4], a in ``along`` (m), b in
    ``across`` (m), psi in ``yaw_deg`` (degrees), k = (ia * len(across) + ib) * len(yaw_deg) + ipsi.  The start pose of
    hypothesis k is ``T_center @ D_k``."""
    along, across, yaw_deg = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (along, across, yaw_deg))
    out = np.tile(np.eye(4), (len(along) * len(across) * len(yaw_deg), 1, 1))
    k = 0
    for a in along:
        for b in across:
            for psi in yaw_deg:
                c, sn = math.cos(math.radians(psi)), math.sin(math.radians(psi))
                out[k, :2, :2] = [[c, 0.0 - sn], [sn, c]]                     # 0.0 - 0.0 is +0.0: psi = 0 gives the identity, bit for bit
                out[k, :2, 3] = [a, b]
                k += 1
    return out


MAX_HYPOTHESES = 64            # SPS_NDT_MAX_HYP
MAX_POSES = 65536              # SPS_NDT_MAX_POSES
MAX_UPDATE_POINTS = 65536      # SPS_NDT_UPDATE_MAX_POINTS
MAX_LEVELS = 4                 # SPS_NDT_PYR_MAX_LEVELS


def _checked_poses(poses, what="poses", most=MAX_POSES, n="P"):
    T = np.ascontiguousarray(np.asarray(poses, dtype=np.float64))
    if T.ndim != 3 or T.shape[1:] != (4, 4) or not 1 <= len(T) <= most or not np.isfinite(T).all():
        raise ValueError(f"{what} must be finite, [{n}, 4, 4] with 1 <= {n} <= {most}")
    return T


def _score_layout(P):
    """offsets (in doubles) of the one float64 buffer of ``score_poses``: score[P][2] | n_points int32 (+ pad)"""
    return _offsets((("score", 2 * P), ("n_points", 1)))


class PendingScores(_Pending):
    """The scores of a pose grid whose work has been issued; ``result()`` -> (scores [P] float64, counts [P] int64)."""

    def __init__(self, n_pose, host, event, keep):
        super().__init__(host, event, keep)
        self._n_pose = n_pose

    def result(self):
        o = _score_layout(self._n_pose)
        sc = self._wait()[o["score"]:o["n_points"]].reshape(self._n_pose, 2)
        return sc[:, 0].copy(), sc[:, 1].astype(np.int64)


@dataclass
class RelocalisationResult:
    scores: np.ndarray         # [P] the NDT score of every pose of the grid
    counts: np.ndarray         # [P] int, the scan points counted at that pose
    candidates: np.ndarray     # [keep] int, indices into the grid by (score descending, index ascending); -1: slot not filled
    batch: BatchPoseResult     # the ``keep`` alignments, hypothesis j started from the pose of candidates[j]
    index: int                 # the grid index of the selected alignment's start pose, or -1 where none was selected
    pose: np.ndarray           # 4x4: batch.pose
    map_update: object = None  # MapUpdateResult of the frame, with integrate=True (batch.map_update)
    map_carve: object = None   # MapCarveResult of the frame, with carve=True (batch.map_carve)

    @property
    def ok(self) -> bool:
        return self.index >= 0


def _search_layout(P, K):
    """offsets (in doubles) of the search's part of a relocalisation's buffer, in front of the batch's:
    score[P][2] | top int32[K] (+ pad) | n_top int32 (+ pad) | T_top[K][16]"""
    return _offsets((("score", 2 * P), ("top", (K + 1) // 2), ("n_top", 1), ("T_top", 16 * K)))


class PendingRelocalisation(_Pending):
    """A pose search and the alignments of its candidates, issued; everything lives on the device until result()."""

    def __init__(self, n_pose, batch_pending):
        super().__init__(batch_pending._host, batch_pending._event, batch_pending._keep)
        self._n_pose, self._batch = n_pose, batch_pending

    def _pose_on_device(self):
        return self._batch._pose_on_device()

    def result(self) -> RelocalisationResult:
        b = self._batch
        K, P = b._n_hyp, self._n_pose
        h, o = self._wait(), _search_layout(P, K)
        sc = h[o["score"]:o["top"]].reshape(P, 2)
        cand = h[o["top"]:o["n_top"]].view(np.int32)[:K].astype(np.int64)
        batch = b._parse(h)
        index = int(cand[batch.best]) if batch.best >= 0 else -1
        return RelocalisationResult(sc[:, 0].copy(), sc[:, 1].astype(np.int64), cand, batch, index, batch.pose, batch.map_update,
                                    batch.map_carve)


GLOBAL_GRID_DEFAULTS = dict(resolution=0.5, map_z=(-math.inf, math.inf), levels=3)


@dataclass
class GlobalSearchResult:
    index: np.ndarray          # [keep] int, leaf ids (a * H + j) * W + i by (score descending, id ascending); -1: slot not filled
    score: np.ndarray          # [keep] int, the slice points of the scan that fall on occupied cells at that leaf
    poses: np.ndarray          # [keep, 4, 4]: Trans(r (i0 + i), r (j0 + j), 0) Rz(2 pi a / yaw_steps) T_up of every leaf
    n_found: int               # slots filled
    certified: int             # the leading results that are the exhaustive ranking's: score > dropped_bound
    dropped_bound: int         # the highest bound of anything the search dropped (-1: nothing was dropped)
    n_dropped: int             # nodes dropped, for min_score or for the frontier
    candidates: np.ndarray     # [levels + 1] int, nodes scored at level l
    kept: np.ndarray           # [levels + 1] int, nodes kept at level l
    n_slice: int               # thinned points inside the scan slice
    n_points: int              # points after thinning
    candidate_lists: list = None   # with trace=True: per level the ids of the candidates, in their order
    kept_lists: list = None        # with trace=True: per level the ids of the kept nodes, in their order

    def leaf(self, k: int, W: int, H: int):
        """(a, j, i) of result k"""
        i, aj = int(self.index[k]) % W, int(self.index[k]) // W
        return aj // H, aj % H, i


def _global_layout(K, trace_words=0):
    """offsets (in doubles) of the global search's part of a buffer: top int32[K] (+ pad) | score int32[K] (+ pad) | n_top
    int32 (+ pad) | info int32[20] | T_top[K][16] | trace int32[trace_words] (+ pad)"""
    return _offsets((("top", (K + 1) // 2), ("score", (K + 1) // 2), ("n_top", 1), ("info", _native.BBS_INFO_WORDS // 2),
                     ("T_top", 16 * K), ("trace", (trace_words + 1) // 2)), (("n_points", 1),))


def _global_result_of(h, K, L, F, trace, n_points) -> GlobalSearchResult:
    o = _global_layout(K, (L + 1) * 5 * F if trace else 0)
    info = h[o["info"]:o["T_top"]].view(np.int32).astype(np.int64)
    per_level = info[4:4 + 2 * (L + 1)].reshape(L + 1, 2)
    cl = kl = None
    if trace:
        tr = h[o["trace"]:o["size"]].view(np.int32)[:(L + 1) * 5 * F].reshape(L + 1, 5 * F).astype(np.int64)
        cl = [tr[l, :4 * F][tr[l, :4 * F] >= 0] for l in range(L + 1)]
        kl = [tr[l, 4 * F:][tr[l, 4 * F:] >= 0] for l in range(L + 1)]
    return GlobalSearchResult(h[o["top"]:o["score"]].view(np.int32)[:K].astype(np.int64),
                              h[o["score"]:o["n_top"]].view(np.int32)[:K].astype(np.int64),
                              h[o["T_top"]:o["trace"]].reshape(K, 4, 4).copy(), int(h[o["n_top"]:o["info"]].view(np.int32)[0]),
                              int(info[0]), int(info[1]), int(info[2]), per_level[:, 0].copy(), per_level[:, 1].copy(),
                              int(info[3]), int(n_points), cl, kl)


class PendingGlobalSearch(_Pending):
    """A global search whose work has been issued; ``result()`` -> GlobalSearchResult."""

    def __init__(self, K, L, F, trace, host, event, keep):
        super().__init__(host, event, keep)
        self._shape = (K, L, F, trace)

    def result(self) -> GlobalSearchResult:
        K, L, F, trace = self._shape
        h = self._wait()
        o = _global_layout(K, (L + 1) * 5 * F if trace else 0)
        return _global_result_of(h, K, L, F, trace, h[o["n_points"]:o["total"]].view(np.int32)[0])


@dataclass
class GlobalLocalisationResult:
    search: GlobalSearchResult # the leaves the registration started from
    batch: BatchPoseResult     # the ``keep`` alignments, hypothesis k started from search.poses[k]
    index: int                 # the leaf id of the selected alignment's start pose, or -1 where none was selected
    pose: np.ndarray           # 4x4: batch.pose
    map_update: object = None  # MapUpdateResult of the frame, with integrate=True (batch.map_update)
    map_carve: object = None   # MapCarveResult of the frame, with carve=True (batch.map_carve)

    @property
    def ok(self) -> bool:
        return self.index >= 0


class PendingGlobalLocalisation(_Pending):
    """A global search and the alignments of its leaves, issued; everything lives on the device until result()."""

    def __init__(self, L, F, batch_pending):
        super().__init__(batch_pending._host, batch_pending._event, batch_pending._keep)
        self._L, self._F, self._batch = L, F, batch_pending

    def _pose_on_device(self):
        return self._batch._pose_on_device()

    def result(self) -> GlobalLocalisationResult:
        h = self._wait()
        batch = self._batch._parse(h)
        search = _global_result_of(h, self._batch._n_hyp, self._L, self._F, False, batch.results[0].n_points)
        index = int(search.index[batch.best]) if batch.best >= 0 else -1
        return GlobalLocalisationResult(search, batch, index, batch.pose, batch.map_update, batch.map_carve)


class PendingMatch(_Pending):
    """A scan-matching status whose work has been issued; ``result()`` -> MatchStatus, with ``distances`` (MatchStatus, d2)."""

    def __init__(self, distances, host, event, keep):
        super().__init__(host, event, keep)
        self._distances = distances

    def result(self):
        h = self._wait()
        m = _match_of(h[:MATCH_WORDS])
        if not self._distances:
            return m
        n = int(h[MATCH_WORDS:MATCH_WORDS + 1].view(np.int32)[0])
        return m, h[MATCH_WORDS + 1:MATCH_WORDS + 1 + n].copy()


class ScanToMapLocaliser:
    """``ScanToMapLocaliser(map_points)(rows, count, T_init)`` -> PoseResult.  The map's uniform grid (cell size =
    ``max_distance``) lives in a native context of the localiser's own, so the grid of the offline item path
    (datasets.blt_dataset.DeviceRadiusSubmap, r = voxel size) is untouched.  ``capacity`` bounds the points that enter
    the alignment: survivors of the thinning beyond it are dropped.

    ``match_status`` (None: nothing is built and nothing changes; a dict with any of ``max_distance`` (0.5), ``max_range``
    (None), ``min_inlier_fraction`` (0.0), ``max_error`` (inf), ``min_valid`` (1); C ABI: "localiser, scan-matching status";
    DESIGN.md 8n): every registration is followed on its stream by the scan-matching status at the pose it hands on -- of the
    thinned points that are finite and within ``max_range`` of the sensor (valid), the share with a map point within
    ``max_distance`` (inliers), and the inliers' mean squared distance -- and the result's ``match`` carries it.  A
    registration with status 0 or 1 whose status misses a threshold is *lost* (verdict ``LOST``), and that verdict, not the
    registration's status, then gates ``integrate``, ``carve`` and ``PoseEstimator.correct_from`` on the device.  The map
    is the localiser's own grid, so ``max_distance`` may not exceed the localiser's."""

    # what only an NDTLocaliser can have: no pyramid, no online map, the scan's points registered as they are
    resolutions = level_iterations = level_capacities = cell_capacity = source_resolutions = None
    source = "points"
    _match_opts = None                                               # no match_status: nothing is built, nothing changes

    def __init__(self, map_points, max_distance: float = 1.0, leaf: float = 0.2, iterations: int = 30,
                 min_correspondences: int = 50, tol_t: float = 1e-4, tol_r: float = 1e-5, device="cuda",
                 capacity: int = 1 << 16, match_status: dict = None):
        if not (math.isfinite(max_distance) and max_distance > 0 and math.isfinite(leaf) and leaf > 0):
            raise ValueError("max_distance and leaf must be finite and > 0")
        self.max_distance = float(max_distance)
        self._match_opts = _checked_match(match_status)
        if self._match_opts is not None and self._match_opts["max_distance"] > self.max_distance:
            raise ValueError("match_status: max_distance must not exceed the localiser's max_distance (its grid's cell)")
        self._open(self._map_xyz(map_points), leaf, iterations, min_correspondences, tol_t, tol_r, device, capacity,
                   _native.lib.sps_loc_align_scratch)

    def _build_map(self, xyz):
        """the localiser's map from the map's points on the device, in its context"""
        from .datasets.blt_dataset import radius_grid_cells
        if self.n_map:
            keys, start, pts = radius_grid_cells(xyz, self.max_distance)
            self.ctx.radius_grid_upload(keys.contiguous().data_ptr(), start.data_ptr(), pts.data_ptr(), xyz.data_ptr(),
                                        len(keys), self.n_map, self.max_distance, self.max_distance, self.stream.cuda_stream)
        else:
            self.ctx.radius_grid_upload(None, None, None, None, 0, 0, self.max_distance, self.max_distance,
                                        self.stream.cuda_stream)

    @staticmethod
    def _map_xyz(map_points) -> np.ndarray:
        """the map's coordinates on the host, contiguous float64 [n, 3] (such an array comes back as it is)"""
        mp = map_points.detach().cpu().numpy() if torch.is_tensor(map_points) else np.asarray(map_points)
        return np.ascontiguousarray(mp[:, :3], dtype=np.float64)

    def _open(self, xyz, leaf, iterations, min_correspondences, tol_t, tol_r, device, capacity, align_scratch_bytes):
        """What both constructors do behind their own checks: the settings both have, the map ``xyz`` (float64 [n, 3] on the
        host) on the device, the native context, ``_build_map``, then the buffer of the thinned points, the alignment's
        scratch and the thinning's"""
        if iterations < 0 or capacity < 1:
            raise ValueError("iterations must be >= 0 and capacity >= 1")
        self.leaf, self.iterations, self.min_correspondences = float(leaf), int(iterations), int(min_correspondences)
        self.tol_t, self.tol_r, self.capacity = float(tol_t), float(tol_r), int(capacity)
        self.device = _device_of(device)
        xyz = torch.as_tensor(xyz).to(self.device)
        self.n_map = len(xyz)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream()
            self.ctx = _native.Context(self.device.index)
            self._build_map(xyz)
            if self._match_opts is not None:
                self._build_match(xyz)
                self._match_scratch = torch.empty(_native.lib.sps_loc_match_status_scratch(self.capacity), dtype=torch.uint8,
                                                  device=self.device)
            self._pts = torch.empty((self.capacity, 3), dtype=torch.float64, device=self.device)
            self._align_scratch = torch.empty(align_scratch_bytes(self.capacity), dtype=torch.uint8, device=self.device)
            self._ds_scratch, self._ds_rows = None, -1

    def _build_match(self, xyz):
        """the map of the scan-matching status: the ICP's own grid, uploaded by ``_build_map``"""

    def _status(self, n_ptr, T_ptr, gate_in_ptr, out_ptr, s, d2_ptr=None):
        """the scan-matching status of self._pts (their count at n_ptr) at the device pose at T_ptr into the MATCH_WORDS words
        at out_ptr, on stream s; ``gate_in_ptr``: the registration's status word, or None"""
        m = self._match_opts
        self.ctx.loc_match_status(self._pts.data_ptr(), n_ptr, self.capacity, T_ptr, gate_in_ptr, m["max_distance"],
                                  -1.0 if m["max_range"] is None else m["max_range"], m["min_inlier_fraction"], m["max_error"],
                                  m["min_valid"], out_ptr, d2_ptr, self._match_scratch.data_ptr(), s)

    @torch.no_grad()
    def match_status_at(self, rows, count, T, distances: bool = False) -> "PendingMatch":
        """The scan-matching status of the rows at any host pose ``T`` (4x4, sensor -> map), ungated: the rows are thinned as
        ``submit`` thins them and compared with the map as every registration of a localiser with ``match_status`` is
        (DESIGN.md 8n).  Issued on the current stream; ``result()`` -> MatchStatus, or with ``distances`` (debug)
        (MatchStatus, float64 [n_points]): per thinned point the squared distance to its nearest map point where it is an
        inlier, inf where it is valid but no inlier, -1 where it is not valid."""
        if self._match_opts is None:
            raise ValueError("match_status_at needs a localiser with match_status")
        rows = self._checked_rows(rows)
        Th = _pose(T)
        if Th is None or not np.isfinite(Th).all():
            raise ValueError("T must be a finite 4x4 matrix")
        o = _offsets((("match", MATCH_WORDS), ("n_points", 1), ("d2", self.capacity if distances else 0)))

        def work(out, n_ptr, T_dev, s):
            base = out.data_ptr()
            self._status(n_ptr, T_dev.data_ptr(), None, base + o["match"] * 8, s, base + o["d2"] * 8 if distances else None)
        return PendingMatch(distances, *self._issue(rows, count, o["total"], o["n_points"] * 8, work,
                                                    np.ascontiguousarray(Th, dtype=np.float64)[None].copy()))

    def _downsample_scratch(self, n_max):
        if n_max > self._ds_rows:                                    # grows with the largest scan seen (stream-ordered reuse)
            rows = max(n_max, 1024)
            self._ds_scratch = torch.empty(_native.lib.sps_loc_downsample_scratch(rows), dtype=torch.uint8, device=self.device)
            self._ds_rows = rows
        return self._ds_scratch

    def _thin(self, rows, n_dev, n_max, n_points_ptr, s):
        """voxel-grid thinning of the rows into self._pts on stream s; the survivors' count goes to n_points_ptr"""
        self.ctx.loc_downsample(rows.data_ptr() if n_max else None, rows.stride(0) if n_max else 3, n_max, n_dev.data_ptr(),
                                self.leaf, self._pts.data_ptr(), self.capacity, n_points_ptr,
                                self._downsample_scratch(n_max).data_ptr(), s)

    @staticmethod
    def _to_host(out, st):
        """the frame's device buffer into a pinned host buffer of its own, behind everything issued on st -> (host, event)"""
        host = torch.empty(out.numel(), dtype=out.dtype).pin_memory()
        host.copy_(out, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(st)
        return host, ev

    def _checked_rows(self, rows):
        if not (torch.is_tensor(rows) and rows.is_cuda and rows.device == self.device):
            raise TypeError(f"{type(self).__name__}.submit needs a tensor on the localiser's device")
        if rows.dim() != 2 or rows.shape[1] < 3:
            raise ValueError(f"rows must be [n, >=3], got {tuple(rows.shape)}")
        if rows.dtype != torch.float32:
            rows = rows.to(torch.float32)
        if rows.shape[0] and rows.stride(1) != 1:
            rows = rows.contiguous()
        return rows

    def _count_on_device(self, count, n_max):
        if torch.is_tensor(count):
            if count.dtype != torch.int32 or count.device != self.device or count.numel() < 1:
                raise TypeError("count must be an int or an int32 tensor on the localiser's device")
            return count
        if not 0 <= int(count) <= n_max:
            raise ValueError(f"count must be in [0, {n_max}], got {count}")
        return torch.full((1,), int(count), dtype=torch.int32, device=self.device)

    @torch.no_grad()
    def submit(self, rows, count, T_init, with_normal: bool = False, iterations: int = None, integrate: bool = False,
               max_cell_points: int = 0, carve: bool = False, carve_options: dict = None) -> PendingPose:
        """rows: device tensor [n_max, >= 3] (float32; other dtypes are converted); count: an int or a device int32 tensor
        holding the number of valid rows; T_init: 4x4.  Issued on the current stream.  ``integrate`` (a localiser with an
        online map only): the thinned points are then folded into the map at the corrected pose, behind the alignment on
        the same stream and only where its status is 0 or 1; the result's ``map_update`` tells what happened.  ``carve``
        (the same localisers; ``carve_options``: the keywords of ``NDTLocaliser.carve``): the thinned points are cast as
        rays from the corrected pose and the map is carved, behind the alignment, under the same gate and before the
        update, so a cell cleared and observed again in one frame is refilled by it; the result's ``map_carve`` tells."""
        self._check_integrate(integrate, max_cell_points)
        copts = self._check_carve(carve, carve_options)
        rows = self._checked_rows(rows)
        T = _pose(T_init)
        if T is None or not np.isfinite(T).all():
            raise ValueError("T_init must be a finite 4x4 matrix")
        K = self.iterations if iterations is None else int(iterations)
        pyramid = self.resolutions is not None
        match = self._match_opts is not None
        n_src_levels = 0 if self.source_resolutions is None else len(self.source_resolutions)
        shape = (K, with_normal, pyramid, None if self.level_capacities is None else len(self.level_capacities), integrate, carve,
                 match, n_src_levels)
        o = _pose_layout(*shape)

        def work(out, n_ptr, _, s):
            base = out.data_ptr()
            T_ptr, gate_ptr = (base + b for b in o["hands_on"])
            status_ptr = base + o["status"] * 8
            kw = dict(level_ptr=base + o["levels"] * 8 if K else None) if pyramid else {}
            self._align(n_ptr, T, K, T_ptr, status_ptr, base + o["trace"] * 8 if K else None,
                        base + o["normal"] * 8 if with_normal and K else None, s, **kw)
            if n_src_levels:                                         # every level's valid source cells: the host picks
                at = 2 * o["sources"]
                out.view(torch.int32)[at:at + n_src_levels].copy_(self._n_src_lv[:, 1])
            elif self.source == "cells":                             # the valid source cells into the pad behind n_points
                at = 2 * o["n_points"] + 1
                out.view(torch.int32)[at:at + 1].copy_(self._n_src[1:2])
            if match:                                                # its verdict is the gate of what follows
                self._status(n_ptr, T_ptr, status_ptr, base + o["match"] * 8, s)
            if carve:
                self._carve(n_ptr, None, T_ptr, gate_ptr, copts, base + o["carve"] * 8, s)
            if integrate:
                self._update(n_ptr, None, T_ptr, gate_ptr, max_cell_points, base + o["update"] * 8, s)
        return PendingPose(K, with_normal, *self._issue(rows, count, o["total"], o["n_points"] * 8, work), *shape[2:])

    def _issue(self, rows, count, size, n_points_at, work, poses=None, dtype=torch.float64):
        """The one path on which every entry point issues its work, on the caller's current stream and with no
        synchronisation: the count on the device, ``poses`` (a host array: through a pinned buffer; a device tensor: as it
        is) on the device, the call's one zeroed device buffer of ``size`` words of ``dtype``, the thinning of the checked
        ``rows`` with the survivors' count at byte ``n_points_at`` of that buffer, then ``work(out, n_ptr, T_dev, s)``, then
        the buffer's copy into a pinned host buffer and the event behind it -> (host, event, keep) for the pending object"""
        n_max, dev = rows.shape[0], self.device
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream()
            n_dev = self._count_on_device(count, n_max)
            T_host, T_dev = None, poses
            if isinstance(poses, np.ndarray):
                T_host = torch.from_numpy(poses).pin_memory()
                T_dev = T_host.to(dev, non_blocking=True)            # on the caller's stream; both stay with the pending object
            out = torch.zeros(size, dtype=dtype, device=dev)
            n_ptr = out.data_ptr() + n_points_at
            self._thin(rows, n_dev, n_max, n_ptr, st.cuda_stream)
            work(out, n_ptr, T_dev, st.cuda_stream)
            host, ev = self._to_host(out, st)
        return host, ev, (rows, n_dev, out, T_host, T_dev)

    def _check_integrate(self, integrate, max_cell_points=0, single_map=False):
        """``single_map``: the caller works on the single map at ``resolution`` (batch, search, ``map_info``), which an
        online pyramid's ``level_capacities`` do not make dynamic"""
        caps = self.level_capacities
        if integrate and caps is None and self.resolutions is not None:
            raise ValueError("integrate needs a single-resolution localiser: the online map has no pyramid")
        if integrate and (caps is None or single_map) and self.cell_capacity is None:
            raise ValueError("integrate needs a localiser with an online map: NDTLocaliser(..., cell_capacity=N)")
        if integrate and int(max_cell_points) < 0:
            raise ValueError("max_cell_points must be >= 0")

    def _check_carve(self, carve, carve_options=None, single_map=False):
        """the carve's options with the defaults filled in (None without ``carve``), before any device work; on an online
        pyramid ``end_margin`` comes back as a tuple, one float per level.  ``single_map``: as for ``_check_integrate``"""
        if not carve:
            if carve_options is not None:
                raise ValueError("carve_options needs carve=True")
            return None
        caps = self.level_capacities
        if caps is None and self.resolutions is not None:
            raise ValueError("carve needs a single-resolution localiser: the online map has no pyramid")
        if (caps is None or single_map) and self.cell_capacity is None:
            raise ValueError("carve needs a localiser with an online map: NDTLocaliser(..., cell_capacity=N)")
        unknown = set(carve_options or ()) - set(CARVE_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown carve options {sorted(unknown)}")
        o = dict(CARVE_DEFAULTS, **(carve_options or {}))
        if caps is not None and not single_map:                      # None: each level's resolution; a scalar: every level
            em = o["end_margin"]
            em = self.resolutions if em is None else (em,) * len(caps) if np.ndim(em) == 0 else tuple(em)
            if len(em) != len(caps):
                raise ValueError("end_margin needs one value per level")
            margins = o["end_margin"] = tuple(float(v) for v in em)
        else:
            if o["end_margin"] is None:
                o["end_margin"] = self.resolution
            o["end_margin"] = float(o["end_margin"])
            margins = (o["end_margin"],)
        o["through_sigma"] = float(o["through_sigma"])
        o["min_pass"], o["miss_frames"], o["max_steps"] = int(o["min_pass"]), int(o["miss_frames"]), int(o["max_steps"])
        if not (all(math.isfinite(v) and v >= 0 for v in margins) and math.isfinite(o["through_sigma"]) and o["through_sigma"] > 0):
            raise ValueError("end_margin must be finite and >= 0, through_sigma finite and > 0")
        if o["min_pass"] < 1 or o["miss_frames"] < 1 or not 1 <= o["max_steps"] <= MAX_CARVE_STEPS:
            raise ValueError(f"min_pass and miss_frames must be >= 1 and max_steps in [1, {MAX_CARVE_STEPS}]")
        return o

    def _align(self, n_ptr, T, K, T_out_ptr, status_ptr, trace_ptr, normal_ptr, s):
        self.ctx.loc_align(self._pts.data_ptr(), n_ptr, self.capacity, T, K, self.min_correspondences, self.tol_t, self.tol_r,
                           T_out_ptr, status_ptr, trace_ptr, normal_ptr, self._align_scratch.data_ptr(), s)

    def submit_filtered(self, pending, T_init, **kw) -> PendingPose:
        """The kept rows of a pending SPSFilter / SPSCVMFilter frame and their device count go straight in, without the
        frame's result()."""
        return self.submit(pending._filtered, pending.count_dev, T_init, **kw)

    def __call__(self, rows, count, T_init, **kw) -> PoseResult:
        return self.submit(rows, count, T_init, **kw).result()


class NDTLocaliser(ScanToMapLocaliser):
    """``NDTLocaliser(map_points)(rows, count, T_init)`` -> PoseResult, by point-to-distribution registration.  The map
    becomes one Gaussian (mean, inverse covariance) per cell of edge ``resolution`` in a native context of the
    localiser's own; a scan point is scored against its own cell and, with ``neighbours=7``, the six face neighbours.
    ``submit``, ``submit_filtered`` and ``__call__`` are ScanToMapLocaliser's.  In the result ``n_corr`` counts the scan
    points with at least one contributing cell, ``trace[:, 1]`` and ``normal[:, 27]`` hold the NDT score
    sum -d1 exp(-d2 s / 2) (larger is better) and ``rmse`` is sqrt(score / n_corr), not a distance.

    ``resolutions`` (None: no pyramid; up to 4 cell edges, strictly decreasing, e.g. ``(2.0, 1.0, 0.5)``): one more static
    map per entry, and ``submit`` / ``submit_filtered`` / ``__call__`` then register coarse to fine in one call.
    ``iterations`` is the budget of slots (one slot = one iteration at some level) and ``level_iterations`` the most slots
    each level may use (None: ``iterations`` each).  A level hands its pose to the next when it converges or has used its
    slots; only the last level's convergence is status 0, and the result's ``levels`` tells the level of every slot.
    Status 2 / 3 at any level are final and give the guess back.  ``submit_batch``, ``submit_from_device`` and
    ``relocalise`` register on the pyramid too when asked with ``coarse_to_fine=True``; without it they,
    ``score_poses`` and ``map_cells`` keep using the single map of edge ``resolution``; ``pyramid_cells(level)`` shows a level.

    ``level_capacities`` (with ``resolutions``; one cell capacity per level, each at least the level's cells): the pyramid's
    levels are online maps, ``integrate`` / ``carve`` and ``submit(..., integrate=True, carve=True)`` work on all of them
    at once and report one result per level; ``pyramid_info(level)`` and ``carve_state(level)`` show a level.  The single
    map stays static, so the batch and the search refuse ``integrate`` and ``carve`` unless they register
    ``coarse_to_fine``: then both work on all levels at the selected pose.  ``capacity`` is then at most 65536.

    ``source="cells"`` registers distribution to distribution: the thinned scan is reduced to one Gaussian per cell of edge
    ``source_resolution`` (default: ``resolution``) of the sensor frame, valid from ``source_min_points`` points (default:
    ``min_points_per_cell``), and these are registered against the map's Gaussians.  ``n_corr`` then counts source cells,
    ``min_correspondences`` bounds them, and the result's ``n_sources`` tells how many valid ones the scan gave.
    ``submit`` / ``submit_filtered`` / ``__call__``, ``integrate`` and ``carve`` work as before (the map still takes the
    thinned points); ``resolutions`` and the global search are refused, and ``submit_batch``, ``submit_from_device``,
    ``score_poses`` and ``relocalise`` are refused unless they are called with ``d2d=True``, which registers and scores the
    scan's cells from poses on the device.  ``capacity`` is then at most 65536.  ``source="points"`` (the
    default) is the point-to-distribution path.

    ``source_resolutions`` (with ``source="cells"`` and ``resolutions``, one finite edge > 0 per level, in no way tied to the
    map's; not with ``source_resolution``) lifts the refusal of ``resolutions``: ``submit`` / ``submit_filtered`` /
    ``__call__`` thin the scan once, build its cells at every level's edge in one set of launches and register them coarse
    to fine against the pyramid in one call.  ``source_min_points`` is then an int for all levels or one
    per level.  The handoff is the pyramid's with one more rule: a level whose valid sources are fewer than
    ``min_correspondences`` is skipped, and the last level that qualifies ends the call as the last level does (level 0 is
    always entered).  ``levels`` is as for points, ``n_sources`` is the valid-cell count of the level of the last live slot,
    and ``source_cells(rows, count, level)`` shows a level.  ``level_capacities`` is allowed: the map still takes the thinned
    points.  The calls with ``d2d=True`` keep working on the single map, with sources at ``resolution`` (valid from
    ``source_min_points`` where that is one int, else from ``min_points_per_cell``).  ``submit_batch``,
    ``submit_from_device`` and ``relocalise`` register the scan's cells on the pyramid too when asked with
    ``d2d_pyramid=True``; ``d2d=True`` with ``coarse_to_fine=True`` and the global search stay refused.

    ``global_grid`` (None: nothing is built; a dict with any of ``resolution`` (0.5), ``map_z`` = (lo, hi) (everything) and
    ``levels`` (3, at most 7)): the map points of that height slice become an occupancy grid of that edge with ``levels``
    pooled levels on the device, and ``global_search`` / ``localise_global`` find the pose with no start pose.
    ``capacity`` is then at most 65536, and ``source="cells"`` is refused.

    ``match_status``: as for ScanToMapLocaliser, behind ``submit``, ``submit_batch``, ``submit_from_device``, ``relocalise``
    and ``localise_global`` (the pose is ``T_best`` for all but the first), on the single map, the pyramid and
    ``source="cells"``.  A radius grid of cell ``max_distance`` over the points given at construction is uploaded into the
    localiser's context for it.  The status is taken against those points, not against an online map's Gaussians: with
    ``update_map`` / ``integrate`` and ``min_inlier_fraction > 0`` the map grows only while that share of the scan still
    matches the prior map."""

    def __init__(self, map_points, resolution: float = 1.0, neighbours: int = 7, leaf: float = 0.2, iterations: int = 30,
                 min_correspondences: int = 50, min_points_per_cell: int = 6, outlier_ratio: float = 0.55,
                 eig_ratio: float = 0.01, tol_t: float = 1e-4, tol_r: float = 1e-5, device="cuda", capacity: int = 1 << 16,
                 cell_capacity: int = None, resolutions=None, level_iterations=None, level_capacities=None,
                 source: str = "points", source_resolution: float = None, source_min_points=None,
                 global_grid: dict = None, match_status: dict = None, source_resolutions=None):
        self._match_opts = _checked_match(match_status)
        self.source_resolutions, self.source_level_min_points, source_min_points = self._checked_source_pyramid(
            source, source_resolution, source_resolutions, source_min_points, min_points_per_cell, resolutions)
        self.source, self.source_resolution, self.source_min_points = self._checked_source(
            source, source_resolution, source_min_points, resolution, min_points_per_cell,
            None if self.source_resolutions is not None else resolutions, capacity)
        if level_capacities is not None and cell_capacity is not None:
            raise ValueError("level_capacities and cell_capacity exclude each other: the single map beside an online pyramid is static")
        self.resolutions, self.level_iterations = self._checked_pyramid(resolutions, level_iterations, cell_capacity)
        xyz = self._map_xyz(map_points)
        self.level_capacities = self._checked_level_capacities(self.resolutions, level_capacities, capacity, xyz)
        if cell_capacity is not None and (int(cell_capacity) < 1 or capacity > MAX_UPDATE_POINTS):
            raise ValueError(f"cell_capacity must be >= 1 and, with it, capacity <= {MAX_UPDATE_POINTS}")
        if not (math.isfinite(resolution) and resolution > 0 and math.isfinite(leaf) and leaf > 0):
            raise ValueError("resolution and leaf must be finite and > 0")
        if neighbours not in (1, 7):
            raise ValueError("neighbours must be 1 or 7")
        if not (0.0 < outlier_ratio < 1.0 and 0.0 < eig_ratio <= 1.0 and min_points_per_cell >= 0):
            raise ValueError("outlier_ratio must be in (0, 1), eig_ratio in (0, 1] and min_points_per_cell >= 0")
        self.resolution, self.neighbours = float(resolution), int(neighbours)
        self.min_points_per_cell, self.outlier_ratio, self.eig_ratio = int(min_points_per_cell), float(outlier_ratio), float(eig_ratio)
        self.cell_capacity = None if cell_capacity is None else int(cell_capacity)
        self._global = self._checked_global_grid(global_grid, xyz, capacity, self.source)
        self._open(xyz, leaf, iterations, min_correspondences, tol_t, tol_r, device, capacity, _native.lib.sps_ndt_align_scratch)
        with torch.cuda.device(self.device):
            if self._global is not None:                             # the occupancy pyramid: G0 from the host, pooled there
                g0 = torch.from_numpy(self._global["G0"]).to(self.device)
                self.ctx.bbs_map_build(g0.data_ptr(), self._global["W"], self._global["H"], self._global["levels"],
                                       self.stream.cuda_stream)
                self._bbs_scratch, self._bbs_shape = None, None
            self._grown = {}                                         # the scratch of the calls with K or P poses: _scratch_for
            if self.source == "cells":                               # the scan's cells, their counts, (cells, valid cells)
                self._src = torch.empty((self.capacity, _native.NDT_SRC_REC), dtype=torch.float64, device=self.device)
                self._src_count = torch.empty(self.capacity, dtype=torch.int32, device=self.device)
                self._n_src = torch.zeros(2, dtype=torch.int32, device=self.device)
                self._src_scratch = torch.empty(_native.lib.sps_ndt_source_scratch(self.capacity), dtype=torch.uint8,
                                                device=self.device)
                self._d2d_scratch = torch.empty(_native.lib.sps_ndt_align_d2d_scratch(self.capacity), dtype=torch.uint8,
                                                device=self.device)
            if self.source_resolutions is not None:                  # the same per level of the pyramid of source cells
                L = len(self.source_resolutions)
                self._src_lv = torch.empty((L, self.capacity, _native.NDT_SRC_REC), dtype=torch.float64, device=self.device)
                self._src_count_lv = torch.empty((L, self.capacity), dtype=torch.int32, device=self.device)
                self._n_src_lv = torch.zeros((L, 2), dtype=torch.int32, device=self.device)
                self._src_lv_scratch = torch.empty(_native.lib.sps_ndt_pyramid_source_scratch(self.capacity, L),
                                                   dtype=torch.uint8, device=self.device)
                self._d2d_pyr_scratch = torch.empty(_native.lib.sps_ndt_pyramid_align_d2d_scratch(self.capacity),
                                                    dtype=torch.uint8, device=self.device)

    def _build_map(self, xyz):
        """the single map at ``resolution``, static or online, and the pyramid's levels beside it"""
        from .datasets.blt_dataset import radius_grid_cells
        self.n_cells, cells = 0, (None, None, None, None)
        if self.n_map:
            keys, start, pts = radius_grid_cells(xyz, self.resolution)
            keys = keys.contiguous()
            self.n_cells, cells = len(keys), (keys.data_ptr(), start.data_ptr(), pts.data_ptr(), xyz.data_ptr())
        args = (*cells, self.n_cells, self.n_map, self.resolution, self.min_points_per_cell, self.eig_ratio)
        if self.cell_capacity is None:
            self.ctx.ndt_map_build(*args, self.stream.cuda_stream)
        else:
            if self.cell_capacity < max(self.n_cells, 1):
                raise ValueError(f"cell_capacity {self.cell_capacity} is below the map's {self.n_cells} cells")
            self.ctx.ndt_map_build_dynamic(*args, self.cell_capacity, self.stream.cuda_stream)
            self._update_scratch = torch.empty(_native.lib.sps_ndt_map_update_scratch(self.capacity), dtype=torch.uint8,
                                               device=self.device)
        self.level_cells = None
        if self.resolutions is not None:
            levels, keep = [], []                                # one radius_grid_cells call per level
            for r in self.resolutions:
                if self.n_map:
                    k, st_, p = radius_grid_cells(xyz, r)
                    k = k.contiguous()
                    keep.append((k, st_, p))
                    levels.append((k.data_ptr(), st_.data_ptr(), p.data_ptr(), len(k), r))
                else:
                    levels.append((None, None, None, 0, r))
            self.level_cells = tuple(lv[3] for lv in levels)
            self.ctx.ndt_pyramid_build(levels, xyz.data_ptr() if self.n_map else None, self.n_map, self.min_points_per_cell,
                                       self.eig_ratio, self.outlier_ratio, self.stream.cuda_stream, self.level_capacities)
            if self.level_capacities is not None:                # excludes cell_capacity: a localiser has one online map
                self._update_scratch = torch.empty(
                    _native.lib.sps_ndt_pyramid_update_scratch(self.capacity, len(self.resolutions)), dtype=torch.uint8,
                    device=self.device)
            self._pyr_scratch = torch.empty(_native.lib.sps_ndt_pyramid_align_scratch(self.capacity), dtype=torch.uint8,
                                            device=self.device)

    def _build_match(self, xyz):
        """the map of the scan-matching status: a radius grid of cell ``max_distance`` over the construction's points, in the
        localiser's context, which has no other"""
        from .datasets.blt_dataset import radius_grid_cells
        d = self._match_opts["max_distance"]
        if self.n_map:
            keys, start, pts = radius_grid_cells(xyz, d)
            self.ctx.radius_grid_upload(keys.contiguous().data_ptr(), start.data_ptr(), pts.data_ptr(), xyz.data_ptr(), len(keys),
                                        self.n_map, d, d, self.stream.cuda_stream)
        else:
            self.ctx.radius_grid_upload(None, None, None, None, 0, 0, d, d, self.stream.cuda_stream)

    @staticmethod
    def _checked_source_pyramid(source, source_resolution, source_resolutions, source_min_points, min_points_per_cell,
                                resolutions):
        """(source_resolutions, the levels' source_min_points, the single map's source_min_points) before any device work:
        the first two are tuples, one entry per level, or None without ``source_resolutions``; the third is what
        ``_checked_source`` takes: ``source_min_points`` where that is not a sequence, else None (its default)"""
        seq = source_min_points is not None and np.ndim(source_min_points) != 0
        if source_resolutions is None:
            if seq:
                raise ValueError("a source_min_points sequence needs source_resolutions")
            return None, None, source_min_points
        if source != "cells" or resolutions is None:
            raise ValueError("source_resolutions needs source='cells' and resolutions: one source resolution per level")
        if source_resolution is not None:
            raise ValueError("source_resolutions and source_resolution exclude each other")
        try:
            n_levels = len(tuple(resolutions))
            res = tuple(float(r) for r in source_resolutions)
            mps = tuple(int(v) for v in source_min_points) if seq else \
                (int(min_points_per_cell if source_min_points is None else source_min_points),) * len(res)
        except TypeError:
            raise ValueError("source_resolutions must be a sequence of numbers") from None
        if len(res) != n_levels or not all(math.isfinite(r) and r > 0 for r in res):
            raise ValueError("source_resolutions needs one finite entry > 0 per level of resolutions")
        if len(mps) != n_levels or min(mps) < 0:
            raise ValueError("a source_min_points sequence needs one entry >= 0 per level of resolutions")
        return res, mps, None if seq else source_min_points

    @staticmethod
    def _checked_source(source, source_resolution, source_min_points, resolution, min_points_per_cell, resolutions, capacity):
        """(source, source_resolution, source_min_points) with the defaults filled in, before any device work"""
        if source not in ("points", "cells"):
            raise ValueError("source must be 'points' or 'cells'")
        if source == "points":
            if source_resolution is not None or source_min_points is not None:
                raise ValueError("source_resolution and source_min_points need source='cells'")
            return source, None, None
        if resolutions is not None:
            raise ValueError("source='cells' and resolutions exclude each other: the pyramid registers points")
        if capacity > MAX_UPDATE_POINTS:
            raise ValueError(f"with source='cells', capacity must be <= {MAX_UPDATE_POINTS}")
        res = float(resolution if source_resolution is None else source_resolution)
        mp = int(min_points_per_cell if source_min_points is None else source_min_points)
        if not (math.isfinite(res) and res > 0 and mp >= 0):
            raise ValueError("source_resolution must be finite and > 0 and source_min_points >= 0")
        return source, res, mp

    _global = None                                                   # no global_grid: nothing is built

    @staticmethod
    def _checked_global_grid(global_grid, xyz, capacity, source="points"):
        """None, or the occupancy grid of the global search, before any device work: dict(resolution, map_z, levels, G0 uint8
        [H, W], i0, j0, W, H).  A map point with map_z[0] <= z <= map_z[1] falls into cell (floor(x / r) - i0, floor(y / r) -
        j0), float64 divisions as the NDT cells are grouped; (i0, j0) is the lowest cell hit ((0, 0) and a 1 x 1 grid of 0
        where the slice holds no point)"""
        if global_grid is None:
            return None
        unknown = set(global_grid) - set(GLOBAL_GRID_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown global_grid entries {sorted(unknown)}")
        if source == "cells":
            raise ValueError("global_grid searches with points: it needs an NDTLocaliser with source='points'")
        g = dict(GLOBAL_GRID_DEFAULTS, **global_grid)
        r, L = float(g["resolution"]), int(g["levels"])
        lo, hi = (float(v) for v in g["map_z"])
        if not (math.isfinite(r) and r > 0) or math.isnan(lo) or math.isnan(hi):
            raise ValueError("global_grid: resolution must be finite and > 0 and map_z must not be NaN")
        if not 0 <= L < _native.BBS_MAX_LEVELS:
            raise ValueError(f"global_grid: levels must be in [0, {_native.BBS_MAX_LEVELS - 1}]")
        if capacity > _native.BBS_MAX_POINTS:
            raise ValueError(f"with global_grid, capacity must be <= {_native.BBS_MAX_POINTS}")
        sel = xyz[(xyz[:, 2] >= lo) & (xyz[:, 2] <= hi)]
        with np.errstate(invalid="ignore"):
            c = np.floor(sel[:, :2] / np.float64(r))
        c = c[np.isfinite(c).all(axis=1)]
        if len(c) and np.abs(c).max() >= (1 << 20):
            raise ValueError("global_grid: the map extent exceeds the grid")
        c = c.astype(np.int64)
        i0, j0 = (int(c[:, 0].min()), int(c[:, 1].min())) if len(c) else (0, 0)
        W, H = (int(c[:, 0].max()) - i0 + 1, int(c[:, 1].max()) - j0 + 1) if len(c) else (1, 1)
        if max(W, H) + (1 << L) - 1 > _native.BBS_MAX_STORE:
            raise ValueError(f"global_grid: {W} x {H} cells with {L} levels exceed {_native.BBS_MAX_STORE} cells per axis")
        G0 = np.zeros((H, W), dtype=np.uint8)
        G0[c[:, 1] - j0, c[:, 0] - i0] = 1
        return dict(resolution=r, map_z=(lo, hi), levels=L, G0=G0, i0=i0, j0=j0, W=W, H=H)

    def _checked_global(self, what, keep, yaw_steps, frontier, min_score, scan_z, T_up):
        """the checks of the global search, before any device work -> (K, A, F, min_score, (lo, hi), T_up, yaw table [A, 2])"""
        self._refuse_cells(what)
        g = self._global
        if g is None:
            raise ValueError(f"{what} needs a localiser with an occupancy grid: NDTLocaliser(..., global_grid=dict(...))")
        K, A, F, ms = int(keep), int(yaw_steps), int(frontier), int(min_score)
        if not 1 <= K <= MAX_HYPOTHESES:
            raise ValueError(f"keep must be in [1, {MAX_HYPOTHESES}]")
        if not (1 <= A <= _native.BBS_MAX_YAWS and 1 <= F <= _native.BBS_MAX_FRONTIER and ms >= 0):
            raise ValueError(f"yaw_steps must be in [1, {_native.BBS_MAX_YAWS}], frontier in [1, {_native.BBS_MAX_FRONTIER}] "
                             "and min_score >= 0")
        if A * g["H"] * g["W"] >= 1 << 31:
            raise ValueError("yaw_steps * H * W overflows the int32 leaf id")
        step = 1 << g["levels"]
        n_root = A * (-(-g["H"] // step)) * (-(-g["W"] // step))
        if n_root > 4 * F:
            raise ValueError(f"{n_root} candidates at level {g['levels']} exceed 4 * frontier = {4 * F}: more levels or a "
                             "larger frontier")
        lo, hi = (-math.inf, math.inf) if scan_z is None else (float(v) for v in scan_z)
        if math.isnan(lo) or math.isnan(hi):
            raise ValueError("scan_z must not be NaN")
        U = np.eye(4) if T_up is None else _pose(T_up)
        if U is None or not np.isfinite(U).all():
            raise ValueError("T_up must be a finite 4x4 matrix")
        ang = 2.0 * np.pi * np.arange(A, dtype=np.float64) / np.float64(A)
        return K, A, F, ms, (lo, hi), U, np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=1))

    def _bbs_scratch_for(self, A, F):
        if self._bbs_shape is None or A > self._bbs_shape[0] or F > self._bbs_shape[1]:    # grows (stream-ordered reuse)
            A0, F0 = self._bbs_shape or (0, 0)
            self._bbs_shape = (max(A, A0), max(F, F0))
            self._bbs_scratch = torch.empty(_native.lib.sps_bbs_search_scratch(self.capacity, *self._bbs_shape),
                                            dtype=torch.uint8, device=self.device)
        return self._bbs_scratch

    def _global_search(self, n_ptr, cs_dev, K, A, F, ms, z, U, base, o, trace, s):
        """the search of self._pts into the search's part of a buffer at ``base`` (layout ``o``), on stream s"""
        g = self._global
        self.ctx.bbs_search(self._pts.data_ptr(), n_ptr, self.capacity, U, g["resolution"], g["i0"], g["j0"], z[0], z[1],
                            cs_dev.data_ptr(), A, F, ms, K, base + o["top"] * 8, base + o["score"] * 8, base + o["T_top"] * 8,
                            base + o["n_top"] * 8, base + o["info"] * 8, base + o["trace"] * 8 if trace else None,
                            self._bbs_scratch_for(A, F).data_ptr(), s)

    @torch.no_grad()
    def global_search(self, rows, count, yaw_steps, keep: int = 8, frontier: int = 16384, min_score: int = 1, scan_z=None,
                      T_up=None, trace: bool = False) -> PendingGlobalSearch:
        """Where on the map is the scan, with no start pose (C ABI: "NDT localiser, global search"): the rows
        are thinned as ``submit`` thins them, moved by ``T_up`` (4x4, default the identity: roll, pitch and height), cut to
        ``scan_z`` = (lo, hi) of that frame (None: everything) and matched against the occupancy grid of ``global_grid`` at
        every cell and each of ``yaw_steps`` headings by branch and bound; a leaf's score is the number of slice points on
        occupied cells.  ``frontier`` bounds the nodes kept per level, ``min_score`` the score of anything kept.
        ``result()`` -> GlobalSearchResult with the best ``keep`` (1..64) leaves; its ``certified`` tells how many of them
        are provably the exhaustive search's.  ``trace`` (debug): the result also lists every level's candidates and kept
        nodes.  Issued on the current stream with no synchronisation."""
        K, A, F, ms, z, U, cs = self._checked_global("global_search", keep, yaw_steps, frontier, min_score, scan_z, T_up)
        rows = self._checked_rows(rows)
        L = self._global["levels"]
        o = _global_layout(K, (L + 1) * 5 * F if trace else 0)

        def work(out, n_ptr, cs_dev, s):
            if trace:
                out[o["trace"]:o["size"]].view(torch.int32).fill_(-1)
            self._global_search(n_ptr, cs_dev, K, A, F, ms, z, U, out.data_ptr(), o, trace, s)
        return PendingGlobalSearch(K, L, F, trace, *self._issue(rows, count, o["total"], o["n_points"] * 8, work, cs))

    @torch.no_grad()
    def localise_global(self, rows, count, yaw_steps, keep: int = 8, frontier: int = 16384, min_score: int = 1, scan_z=None,
                        T_up=None, with_normal: bool = False, iterations: int = None, integrate: bool = False,
                        max_cell_points: int = 0, carve: bool = False, carve_options: dict = None,
                        coarse_to_fine: bool = False) -> PendingGlobalLocalisation:
        """``global_search``, then the registration of its ``keep`` leaves as ``submit_batch`` registers start poses and the
        choice among the end poses as it chooses: the leaves' poses stay on the device, as the candidates of ``relocalise``
        do.  ``result()`` -> GlobalLocalisationResult.  ``with_normal`` ... ``coarse_to_fine``: as for ``submit_batch``."""
        K, A, F, ms, z, U, cs = self._checked_global("localise_global", keep, yaw_steps, frontier, min_score, scan_z, T_up)
        rows, copts = self._checked_for_batch("localise_global", rows, integrate, max_cell_points, carve, carve_options,
                                              coarse_to_fine)
        I = self.iterations if iterations is None else int(iterations)
        shape = self._batch_shape(integrate, carve, coarse_to_fine)
        so, o = _global_layout(K), _batch_layout(K, I, with_normal, *shape)

        def work(out, n_ptr, cs_dev, s):
            sbase = out.data_ptr()
            self._global_search(n_ptr, cs_dev, K, A, F, ms, z, U, sbase, so, False, s)
            self._align_batch(n_ptr, sbase + so["T_top"] * 8, K, I, with_normal, sbase + so["size"] * 8, o, s, integrate,
                              max_cell_points, copts, coarse_to_fine)
        issued = self._issue(rows, count, so["size"] + o["total"], (so["size"] + o["n_points"]) * 8, work, cs)
        return PendingGlobalLocalisation(self._global["levels"], F,
                                         PendingPoses(K, I, with_normal, *issued, so["size"], *shape))

    def localise_global_filtered(self, pending, yaw_steps, **kw) -> PendingGlobalLocalisation:
        """``localise_global`` of the kept rows of a pending SPSFilter / SPSCVMFilter frame, without the frame's result()."""
        return self.localise_global(pending._filtered, pending.count_dev, yaw_steps, **kw)

    def global_level(self, level: int) -> np.ndarray:
        """Debug: level ``level`` of the occupancy pyramid as the device stores it, uint8 [H + pad, W + pad] with pad =
        2^levels - 1 and G_level(x, y) at [y + pad, x + pad].  Synchronises."""
        g = self._global
        if g is None:
            raise ValueError("global_level needs a localiser with an occupancy grid: NDTLocaliser(..., global_grid=dict(...))")
        pad = (1 << g["levels"]) - 1
        with torch.cuda.device(self.device):
            out = torch.zeros((g["H"] + pad, g["W"] + pad), dtype=torch.uint8, device=self.device)
            self.ctx.bbs_map_level(level, out.data_ptr())
        return out.cpu().numpy()

    def _refuse_cells(self, what, hint=""):
        if self.source == "cells":
            raise ValueError(f"{what} registers points: it needs an NDTLocaliser with source='points'{hint}")

    def _checked_d2d(self, what, d2d, coarse_to_fine=False):
        """the checks of the ``d2d`` keyword of the calls that take several poses, before any device work: without it a
        cells localiser refuses them as ever, with it the localiser must register cells, and on the single map"""
        if not d2d:
            self._refuse_cells(what, " (or d2d=True, which registers the scan's cells)")
            return False
        if self.source != "cells":
            raise ValueError(f"{what}: d2d=True needs an NDTLocaliser with source='cells'")
        if coarse_to_fine:
            raise ValueError(f"{what}: d2d=True and coarse_to_fine exclude each other: the pyramid registers points here "
                             "(source cells go coarse to fine through submit, with source_resolutions, and from several "
                             "poses with d2d_pyramid=True)")
        return True

    def _checked_d2d_pyramid(self, what, d2d_pyramid, d2d=False, coarse_to_fine=False):
        """the checks of the ``d2d_pyramid`` keyword, before any device work -> whether it is set: it needs the pyramid of
        source cells and stands alone"""
        if not d2d_pyramid:
            return False
        if d2d or coarse_to_fine:
            raise ValueError(f"{what}: d2d_pyramid=True excludes d2d and coarse_to_fine: it registers the scan's cells coarse "
                             "to fine by itself")
        if self.source != "cells" or self.source_resolutions is None:
            raise ValueError(f"{what}: d2d_pyramid=True needs an NDTLocaliser with source='cells' and source_resolutions")
        return True

    @staticmethod
    def _checked_pyramid(resolutions, level_iterations, cell_capacity):
        """(resolutions as a tuple of floats or None, level_iterations as a tuple of ints or None), before any device work"""
        if resolutions is None:
            if level_iterations is not None:
                raise ValueError("level_iterations needs resolutions")
            return None, None
        if cell_capacity is not None:
            raise ValueError("resolutions and cell_capacity exclude each other: the online map is single-resolution")
        res = tuple(float(r) for r in resolutions)
        if not 1 <= len(res) <= MAX_LEVELS:
            raise ValueError(f"resolutions must have 1 to {MAX_LEVELS} entries")
        if not all(math.isfinite(r) and r > 0 for r in res) or any(b >= a for a, b in zip(res, res[1:])):
            raise ValueError("resolutions must be finite, > 0 and strictly decreasing")
        if level_iterations is None:
            return res, None
        caps = tuple(int(v) for v in level_iterations)
        if len(caps) != len(res) or min(caps) < 1:
            raise ValueError("level_iterations needs one entry >= 1 per resolution")
        return res, caps

    @staticmethod
    def _checked_level_capacities(resolutions, level_capacities, capacity, map_points):
        """level_capacities as a tuple of ints or None, before any device work: the cells of every level are counted on the
        host, floor(v / r) in float64 as radius_grid_cells and the kernels divide"""
        if level_capacities is None:
            return None
        if resolutions is None:
            raise ValueError("level_capacities needs resolutions")
        caps = tuple(int(v) for v in level_capacities)
        if len(caps) != len(resolutions):
            raise ValueError("level_capacities needs one entry per resolution")
        if min(caps) < 1:
            raise ValueError("level_capacities must be >= 1")
        if capacity > MAX_UPDATE_POINTS:
            raise ValueError(f"with level_capacities, capacity must be <= {MAX_UPDATE_POINTS}")
        xyz = ScanToMapLocaliser._map_xyz(map_points)
        for l, (r, c) in enumerate(zip(resolutions, caps)):
            n = len(np.unique(np.floor(xyz / np.float64(r)).astype(np.int64), axis=0)) if len(xyz) else 0
            if c < n:
                raise ValueError(f"level_capacities[{l}] = {c} is below the {n} cells of the map at {r} m")
        return caps

    def _scan(self, n_ptr, cells, levels=False):
        """What a call registers, chosen once: the thinned points in self._pts (their count at n_ptr) or, ``cells``, the
        source cells that the caller has built (``levels``: those of every level of ``source_resolutions``) -> (array,
        count pointer); ``d2d=cells`` picks the entry point of ``_native.Context``"""
        if not cells:
            return self._pts.data_ptr(), n_ptr
        src, n_src = (self._src_lv, self._n_src_lv) if levels else (self._src, self._n_src)
        return src.data_ptr(), n_src.data_ptr()

    def _scratch_for(self, scratch_fn, size):
        """the scratch that ``scratch_fn`` of the library sizes for ``size`` hypotheses or poses: one buffer per function
        (by its name: ctypes function pointers do not hash), which grows with the largest size seen (stream-ordered reuse)"""
        buf, seen = self._grown.get(scratch_fn.__name__, (None, 0))
        if size > seen:
            buf = torch.empty(scratch_fn(self.capacity, size), dtype=torch.uint8, device=self.device)
            self._grown[scratch_fn.__name__] = (buf, size)
        return buf

    def _align(self, n_ptr, T, K, T_out_ptr, status_ptr, trace_ptr, normal_ptr, s, level_ptr=None):
        cells, pyramid = self.source == "cells", self.resolutions is not None
        if cells:                                                    # at every level where the pyramid registers them
            (self._build_level_sources if pyramid else self._build_sources)(n_ptr, s)
        elems, count = self._scan(n_ptr, cells, pyramid)
        if pyramid:
            caps = self.level_iterations or (max(K, 1),) * len(self.resolutions)
            scratch = self._d2d_pyr_scratch if cells else self._pyr_scratch
            self.ctx.ndt_pyramid_align(elems, count, self.capacity, T, K, caps, self.neighbours, self.min_correspondences,
                                       self.tol_t, self.tol_r, T_out_ptr, status_ptr, trace_ptr, normal_ptr, level_ptr,
                                       scratch.data_ptr(), s, d2d=cells)
            return
        scratch = self._d2d_scratch if cells else self._align_scratch
        self.ctx.ndt_align(elems, count, self.capacity, T, K, self.neighbours, self.min_correspondences, self.outlier_ratio,
                           self.tol_t, self.tol_r, T_out_ptr, status_ptr, trace_ptr, normal_ptr, scratch.data_ptr(), s, d2d=cells)

    def _build_sources(self, n_ptr, s):
        """the cells of the thinned points in self._pts (their count at n_ptr) into self._src, on stream s"""
        self.ctx.ndt_source_build(self._pts.data_ptr(), n_ptr, self.capacity, self.source_resolution, self.source_min_points,
                                  self.eig_ratio, self._src.data_ptr(), self._src_count.data_ptr(), self._n_src.data_ptr(),
                                  self._src_scratch.data_ptr(), s)

    def _build_level_sources(self, n_ptr, s):
        """the same at every level of ``source_resolutions`` into self._src_lv, in one set of launches"""
        self.ctx.ndt_pyramid_source_build(self._pts.data_ptr(), n_ptr, self.capacity, self.source_resolutions,
                                          self.source_level_min_points, self.eig_ratio, self._src_lv.data_ptr(),
                                          self._src_count_lv.data_ptr(), self._n_src_lv.data_ptr(),
                                          self._src_lv_scratch.data_ptr(), s)

    @torch.no_grad()
    def source_cells(self, rows, count, level: int = 0):
        """Debug (``source="cells"``): the thinning plus the source build of ``submit`` -> dict(mean [C, 3], cov [C, 6] as
        (xx, xy, xz, yy, yz, zz), count int32 [C], valid bool [C]) in the order of the cells' lowest points, as numpy arrays.
        With ``source_resolutions``: the cells of level ``level`` of the pyramid of source cells.  Synchronises."""
        if self.source != "cells":
            raise ValueError("source_cells needs an NDTLocaliser with source='cells'")
        levels = self.source_resolutions
        if not 0 <= int(level) < (1 if levels is None else len(levels)):
            raise ValueError(f"level must be in [0, {1 if levels is None else len(levels)})")
        rows = self._checked_rows(rows)
        n_max = rows.shape[0]
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream()
            n_dev = self._count_on_device(count, n_max)
            n_pts = torch.zeros(2, dtype=torch.int32, device=self.device)
            self._thin(rows, n_dev, n_max, n_pts.data_ptr(), st.cuda_stream)
            if levels is None:
                self._build_sources(n_pts.data_ptr(), st.cuda_stream)
                n_src, src, src_count = self._n_src, self._src, self._src_count
            else:
                self._build_level_sources(n_pts.data_ptr(), st.cuda_stream)
                n_src, src, src_count = (a[int(level)] for a in (self._n_src_lv, self._src_lv, self._src_count_lv))
            C = int(n_src.cpu()[0])                                  # synchronises
            rec = src[:C].cpu().numpy()
            cnt = src_count[:C].cpu().numpy()
        return dict(mean=rec[:, 0:3].copy(), cov=rec[:, 3:9].copy(), count=cnt, valid=rec[:, 9] != 0.0)

    # the online map or, with level_capacities, every level of the online pyramid (then info_ptr: int32[L][4])
    def _update(self, n_ptr, T_host, T_dev_ptr, gate_ptr, max_cell_points, info_ptr, s):
        self.ctx._ndt_update(self.level_capacities is not None, self._pts.data_ptr(), n_ptr, self.capacity, T_host, T_dev_ptr,
                             gate_ptr, max_cell_points, info_ptr, self._update_scratch.data_ptr(), s)

    def _carve(self, n_ptr, T_host, T_dev_ptr, gate_ptr, o, info_ptr, s):
        self.ctx._ndt_carve(self.level_capacities is not None, self._pts.data_ptr(), n_ptr, self.capacity, T_host, T_dev_ptr,
                            gate_ptr, o["end_margin"], o["through_sigma"], o["min_pass"], o["miss_frames"], o["max_steps"],
                            info_ptr, None, s)

    @torch.no_grad()
    def carve(self, rows, count, T, end_margin=None, through_sigma: float = 1.0, min_pass: int = 2, miss_frames: int = 3,
              max_steps: int = 512) -> PendingMapCarve:
        """Carve the online map with the rows as ray ends seen from the host pose ``T`` (4x4, sensor -> map): they are
        thinned with the localiser's ``leaf`` as ``submit`` thins them; every ray gives the cell it ends in a hit and walks
        the cells from the sensor to ``end_margin`` (None: ``resolution``) before its end, at most ``max_steps`` of them,
        and passes through a valid cell where it comes within ``through_sigma`` standard deviations of the cell's Gaussian.
        A cell with no hit and at least ``min_pass`` passing rays was seen through; ``miss_frames`` such frames on end clear
        it (count 0, not valid) until an update refills it; a hit starts the count again.  Issued on the current stream;
        ``result()`` -> MapCarveResult.  An online pyramid (``level_capacities``) carves every level in the same launches:
        ``end_margin`` is then None (each level's resolution), one value for all levels or one per level, and ``result()``
        gives a tuple of MapCarveResult, coarsest level first."""
        o = self._check_carve(True, dict(end_margin=end_margin, through_sigma=through_sigma, min_pass=min_pass,
                                         miss_frames=miss_frames, max_steps=max_steps))
        return self._map_op(rows, count, T, self._carve, o, PendingMapCarve)

    def _map_op(self, rows, count, T, op, options, pending):
        """``op`` (``_carve`` or ``_update``, with its ``options``) on the thinned rows at the host pose ``T``, ungated, into a
        small int32 buffer of its own -> ``pending`` of it"""
        rows = self._checked_rows(rows)
        Th = _pose(T)
        if Th is None or not np.isfinite(Th).all():
            raise ValueError("T must be a finite 4x4 matrix")
        L = None if self.level_capacities is None else len(self.level_capacities)
        o = _map_op_layout(L)

        def work(out, n_ptr, _, s):
            op(n_ptr, Th, None, None, options, out.data_ptr() + o["info"] * 4, s)
        return pending(*self._issue(rows, count, o["total"], o["n_points"] * 4, work, dtype=torch.int32), L)

    def carve_state(self, level: int = None):
        """Debug: (pass, hit, miss) int32 arrays of the online map's assigned cells, in the order of ``map_cells()``: the
        rays that passed through and that ended in every cell in the last carve whose gate was open, and the consecutive
        carves in which the cell was seen through.  ``level``: of that level of an online pyramid instead, in the order of
        ``pyramid_cells(level)``.  Synchronises."""
        if level is not None:
            level = self._checked_online_level(level)
        else:
            self._check_carve(True, single_map=True)
        C = self.cell_capacity if level is None else self.level_capacities[level]
        with torch.cuda.device(self.device):
            out = torch.zeros((3, C), dtype=torch.int32, device=self.device)
            self.ctx._ndt_level_call("carve_cells", level, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        n = self.ctx._ndt_info(level)[0]
        h = out.cpu().numpy()
        return h[0, :n].copy(), h[1, :n].copy(), h[2, :n].copy()

    @torch.no_grad()
    def integrate(self, rows, count, T, max_cell_points: int = 0) -> PendingMapUpdate:
        """Fold the rows into the online map at the host pose ``T`` (4x4, sensor -> map): they are thinned with the
        localiser's ``leaf`` as ``submit`` thins them, then every point joins the moments of its cell; cells the map does
        not have yet are founded while ``cell_capacity`` lasts.  ``max_cell_points`` (0: off) caps the weight of a cell's
        history, so that a changed scene is forgotten.  Issued on the current stream; ``result()`` -> MapUpdateResult.  An
        online pyramid (``level_capacities``) updates every level in the same launches, each within its own capacity, and
        ``result()`` gives a tuple of MapUpdateResult, coarsest level first."""
        self._check_integrate(True, max_cell_points)
        return self._map_op(rows, count, T, self._update, max_cell_points, PendingMapUpdate)

    def map_info(self):
        """Debug: (cells assigned, cell capacity, cells dropped for capacity since the build) of the online map; synchronises."""
        self._check_integrate(True, single_map=True)
        return self.ctx._ndt_info(None)

    def _checked_online_level(self, level):
        if self.level_capacities is None:
            raise ValueError("needs a localiser with an online pyramid: NDTLocaliser(..., resolutions=..., level_capacities=...)")
        if not 0 <= int(level) < len(self.level_capacities):
            raise ValueError(f"level must be in [0, {len(self.level_capacities)})")
        return int(level)

    def pyramid_info(self, level: int):
        """Debug: ``map_info()`` of level ``level`` of an online pyramid (0: the coarsest); synchronises."""
        level = self._checked_online_level(level)
        return self.ctx._ndt_info(level)

    @torch.no_grad()
    def submit_batch(self, rows, count, T_inits, with_normal: bool = False, iterations: int = None, integrate: bool = False,
                     max_cell_points: int = 0, carve: bool = False, carve_options: dict = None,
                     coarse_to_fine: bool = False, d2d: bool = False, d2d_pyramid: bool = False) -> PendingPoses:
        """``submit`` from the K start poses ``T_inits`` [K, 4, 4] (1 <= K <= 64) at once: the scan is thinned once, every
        hypothesis is registered as ``submit`` would register it from its pose, and the hypothesis with the highest NDT
        score at its final pose is selected among those with status 0 / 1 and at least ``min_correspondences`` points
        counted there (equal scores: the lowest index).  Issued on the current stream; ``result()`` -> BatchPoseResult.
        ``integrate`` and ``carve``: as for ``submit``, at the selected pose and only where a hypothesis was selected.

        ``coarse_to_fine`` (a localiser with ``resolutions``; False: the single map at ``resolution``, as ever): every
        hypothesis is registered on the pyramid, as ``submit`` registers there (C ABI: "NDT localiser, pyramid, several
        hypotheses").  ``iterations`` is then the budget of slots and the caps are ``level_iterations`` or
        that budget per level; ``results[k].levels`` tells the level of every slot of hypothesis k and ``iterations`` counts
        its slots; the final scores are taken on the finest level, however far a hypothesis got.  On an online pyramid
        ``integrate`` and ``carve`` then work on all levels at the selected pose, and their results are tuples, one entry
        per level.

        ``d2d`` (a localiser with ``source="cells"``, which refuses the call without it; not with ``coarse_to_fine``): the
        scan is thinned and its source cells are built once, as ``submit`` builds them, and every hypothesis is registered
        distribution to distribution, as ``submit`` registers there (C ABI: "NDT localiser, distribution to distribution,
        several poses").  ``n_corr``, ``counts`` and ``min_correspondences`` then mean source cells and every
        hypothesis' result carries ``n_sources``; ``integrate`` and ``carve`` still work on the thinned points.

        ``d2d_pyramid`` (a localiser with ``source="cells"`` and ``source_resolutions``; not with ``d2d`` or
        ``coarse_to_fine``): the scan is thinned once, its source cells are built at every level and every hypothesis is
        registered coarse to fine distribution to distribution, as ``submit`` registers there (C ABI: "NDT localiser,
        distribution to distribution, pyramid, several hypotheses").  The final scores are taken on the last
        level that the scan's cells do not skip, ``score_level`` of the result, whose valid source cells are its
        ``n_sources``; ``results[k].n_sources`` is, as for ``submit``, the count of the level of hypothesis k's last live
        slot.  ``iterations``, the caps, ``levels``, ``integrate`` and ``carve`` are those of ``coarse_to_fine``."""
        pyr = self._checked_d2d_pyramid("submit_batch", d2d_pyramid, d2d, coarse_to_fine)
        if d2d:                                                      # poses first: they need no device
            self._checked_d2d("submit_batch", d2d, coarse_to_fine)
        if d2d or pyr:
            _checked_poses(T_inits, "T_inits", MAX_HYPOTHESES, "K")
        rows, copts = self._checked_for_batch("submit_batch", rows, integrate, max_cell_points, carve, carve_options,
                                              coarse_to_fine, d2d, pyr)
        T = _checked_poses(T_inits, "T_inits", MAX_HYPOTHESES, "K")
        return self._issue_batch(rows, count, T, len(T), with_normal, iterations, integrate, max_cell_points, copts,
                                 coarse_to_fine or pyr, d2d or pyr)

    @torch.no_grad()
    def submit_from_device(self, rows, count, T_init_dev, with_normal: bool = False, iterations: int = None,
                           integrate: bool = False, max_cell_points: int = 0, carve: bool = False,
                           carve_options: dict = None, coarse_to_fine: bool = False, d2d: bool = False,
                           d2d_pyramid: bool = False) -> PendingPoses:
        """``submit_batch`` with one hypothesis whose start pose is already on the device: ``T_init_dev`` holds 16 contiguous
        float64 entries (a row-major 4 x 4, e.g. ``PoseEstimator.pose_dev``) that work issued earlier on the current stream
        may still be writing.  The host never sees the pose; hypothesis 0 of the result is what ``submit`` gives from the
        same pose, bit for bit.  A pose that is not finite ends as such a pose does in ``sps_ndt_align_batch``.
        ``coarse_to_fine``: as for ``submit_batch``; hypothesis 0 is then what ``submit`` gives on the pyramid.
        ``d2d``: as for ``submit_batch``; hypothesis 0 is then what ``submit`` gives on a ``source="cells"`` localiser.
        ``d2d_pyramid``: as for ``submit_batch``; hypothesis 0 is then what ``submit`` gives on a localiser with
        ``source_resolutions``."""
        pyr = self._checked_d2d_pyramid("submit_from_device", d2d_pyramid, d2d, coarse_to_fine)
        rows, copts = self._checked_for_batch("submit_from_device", rows, integrate, max_cell_points, carve, carve_options,
                                              coarse_to_fine, d2d, pyr)
        T_dev = T_init_dev
        if not (torch.is_tensor(T_dev) and T_dev.is_cuda and T_dev.device == self.device and T_dev.dtype == torch.float64
                and T_dev.numel() == 16 and T_dev.is_contiguous()):
            raise TypeError("T_init_dev must be 16 contiguous float64 entries on the localiser's device")
        return self._issue_batch(rows, count, T_dev, 1, with_normal, iterations, integrate, max_cell_points, copts,
                                 coarse_to_fine or pyr, d2d or pyr)

    def _checked_for_batch(self, what, rows, integrate, max_cell_points, carve, carve_options, coarse_to_fine=False, d2d=False,
                           d2d_pyramid=False):
        """the checks of everything that registers from poses on the device, in their order -> (the checked rows, the carve's
        options).  Without ``coarse_to_fine`` the work is on the single map; with it on the pyramid, which must exist and
        whose levels ``integrate`` and ``carve`` then mean; ``d2d``: the scan's cells are registered (``_checked_d2d``);
        ``d2d_pyramid``: the scan's cells on the pyramid (``_checked_d2d_pyramid``), whose levels the map work then means"""
        if self._checked_d2d_pyramid(what, d2d_pyramid, d2d, coarse_to_fine):
            coarse_to_fine = True
        else:
            self._checked_d2d(what, d2d, coarse_to_fine)
        if coarse_to_fine and self.resolutions is None:
            raise ValueError("coarse_to_fine needs a localiser with a pyramid: NDTLocaliser(..., resolutions=...)")
        self._check_integrate(integrate, max_cell_points, single_map=not coarse_to_fine)
        copts = self._check_carve(carve, carve_options, single_map=not coarse_to_fine)
        return self._checked_rows(rows), copts

    def _batch_shape(self, integrate, carve, coarse_to_fine, d2d=False):
        """the last arguments of ``_batch_layout`` and of ``PendingPoses``; ``coarse_to_fine`` with ``d2d``: the scan's cells
        on the pyramid (``d2d_pyramid``), whose levels' valid source cells ride in the buffer"""
        online = coarse_to_fine and self.level_capacities is not None
        shape = (integrate, carve, bool(coarse_to_fine), len(self.level_capacities) if online else None,
                 self._match_opts is not None)
        # The scoring level is found twice: on the device by the call (NdtCells::last, from cap_src and min_corr) and on the
        # host by ``_scoring_level`` from the two values below.  They must be the cap_src and the min_corr that
        # ``_align_batch`` hands to ``ndt_pyramid_align_batch``: self.capacity and self.min_correspondences.
        if coarse_to_fine and d2d:
            shape += ((len(self.source_resolutions), self.capacity, self.min_correspondences),)
        return shape

    def _issue_batch(self, rows, count, poses, K, with_normal, iterations, integrate, max_cell_points, copts,
                     coarse_to_fine=False, d2d=False):
        """the batch of the K start poses ``poses``: a host array [K, 4, 4], or 16 float64 entries on the device (K = 1);
        ``d2d``: of the scan's source cells, which are built first (with ``coarse_to_fine``: at every level)"""
        I = self.iterations if iterations is None else int(iterations)
        shape = self._batch_shape(integrate, copts is not None, coarse_to_fine, d2d)
        o = _batch_layout(K, I, with_normal, *shape)

        def work(out, n_ptr, T_dev, s):
            if d2d and coarse_to_fine:
                self._level_sources_for_batch(out, n_ptr, o["sources"], s)
            elif d2d:
                self._sources_for_batch(out, n_ptr, o["n_points"], s)
            self._align_batch(n_ptr, T_dev.data_ptr(), K, I, with_normal, out.data_ptr(), o, s, integrate, max_cell_points, copts,
                              coarse_to_fine, d2d)
        return PendingPoses(K, I, with_normal, *self._issue(rows, count, o["total"], o["n_points"] * 8, work, poses), 0, *shape)

    def submit_filtered_batch(self, pending, T_inits, **kw) -> PendingPoses:
        """``submit_batch`` of the kept rows of a pending SPSFilter / SPSCVMFilter frame, without the frame's result()."""
        return self.submit_batch(pending._filtered, pending.count_dev, T_inits, **kw)

    def _align_batch(self, n_ptr, T_ptr, K, I, with_normal, base, o, s, integrate=False, max_cell_points=0, carve_opts=None,
                     coarse_to_fine=False, d2d=False):
        """the K alignments of self._pts from the device poses at T_ptr into the batch's buffer at ``base`` (layout ``o``), on
        the single map or, ``coarse_to_fine``, on the pyramid; ``carve_opts``: then the carve at the selected pose, its info
        words last; ``integrate``: then the map update at the selected pose, its info words behind the batch's part;
        ``d2d``: the K alignments are those of the source cells in self._src (with ``coarse_to_fine``: of every level's in
        self._src_lv), which the caller has built"""
        trace_ptr, normal_ptr = base + o["trace"] * 8 if I else None, base + o["normal"] * 8 if with_normal and I else None
        if coarse_to_fine:
            caps = self.level_iterations or (max(I, 1),) * len(self.resolutions)
            elems, count = self._scan(n_ptr, d2d, True)
            lib = _native.lib
            scratch = self._scratch_for(lib.sps_ndt_pyramid_align_d2d_batch_scratch if d2d
                                        else lib.sps_ndt_pyramid_align_batch_scratch, K)
            self.ctx.ndt_pyramid_align_batch(elems, count, self.capacity, T_ptr, K, I, caps, self.neighbours,
                                             self.min_correspondences, self.tol_t, self.tol_r, base + o["T_out"] * 8,
                                             base + o["status"] * 8, trace_ptr, normal_ptr, base + o["levels"] * 8 if I else None,
                                             base + o["final"] * 8, base + o["best"] * 8, base + o["T_best"] * 8,
                                             scratch.data_ptr(), s, d2d=d2d)
        else:
            elems, count = self._scan(n_ptr, d2d)
            lib = _native.lib
            scratch = self._scratch_for(lib.sps_ndt_align_d2d_batch_scratch if d2d else lib.sps_ndt_align_batch_scratch, K)
            self.ctx.ndt_align_batch(elems, count, self.capacity, T_ptr, K, I, self.neighbours, self.min_correspondences,
                                     self.outlier_ratio, self.tol_t, self.tol_r, base + o["T_out"] * 8, base + o["status"] * 8,
                                     trace_ptr, normal_ptr, base + o["final"] * 8, base + o["best"] * 8,
                                     base + o["T_best"] * 8, scratch.data_ptr(), s, d2d=d2d)
        T_best, gate_ptr = (base + b for b in o["hands_on"])
        if self._match_opts is not None:                             # its verdict is the gate of what follows
            self._status(n_ptr, T_best, base + o["best"] * 8 + 4, base + o["match"] * 8, s)
        if carve_opts is not None:
            self._carve(n_ptr, None, T_best, gate_ptr, carve_opts, base + o["carve"] * 8, s)
        if integrate:
            self._update(n_ptr, None, T_best, gate_ptr, max_cell_points, base + o["update"] * 8, s)

    def _sources_for_batch(self, out, n_ptr, n_points_at, s):
        """``_build_sources`` for a d2d=True call, and the count of valid source cells into the pad behind the n_points
        word (double ``n_points_at`` of ``out``)"""
        self._build_sources(n_ptr, s)
        at = 2 * n_points_at + 1
        out.view(torch.int32)[at:at + 1].copy_(self._n_src[1:2])

    def _level_sources_for_batch(self, out, n_ptr, sources_at, s):
        """``_build_level_sources`` for a d2d_pyramid=True call, and every level's count of valid source cells into the
        ``sources`` part of the batch's buffer (double ``sources_at`` of ``out``)"""
        self._build_level_sources(n_ptr, s)
        at, L = 2 * sources_at, len(self.source_resolutions)
        out.view(torch.int32)[at:at + L].copy_(self._n_src_lv[:, 1])

    def _score(self, T_dev, P, n_points_ptr, score_ptr, s, d2d=False):
        """the scores of the P poses of T_dev for the thinned points in self._pts (their count at n_points_ptr) or, ``d2d``,
        for the source cells in self._src, which the caller has built"""
        elems, count = self._scan(n_points_ptr, d2d)
        scratch = self._scratch_for(_native.lib.sps_ndt_score_d2d_scratch if d2d else _native.lib.sps_ndt_score_scratch, P)
        self.ctx.ndt_score_poses(elems, count, self.capacity, T_dev.data_ptr(), P, self.neighbours, self.outlier_ratio,
                                 score_ptr, scratch.data_ptr(), s, d2d=d2d)

    @torch.no_grad()
    def score_poses(self, rows, count, poses, d2d: bool = False) -> PendingScores:
        """The NDT score and the points counted at each of the P poses ``poses`` [P, 4, 4] (1 <= P <= 65536), with no
        alignment: the scan is thinned once as ``submit`` thins it, and pose p scores what ``submit_batch`` reports as the
        final score of a hypothesis that starts there with ``iterations=0``, bit for bit.  Issued on the current stream.
        ``d2d``: as for ``submit_batch``: the D2D score and the source cells counted, bit for bit what
        ``submit_batch(..., iterations=0, d2d=True)`` reports."""
        if self._checked_d2d("score_poses", d2d):                    # poses first: they need no device
            _checked_poses(poses)
        rows = self._checked_rows(rows)
        T = _checked_poses(poses)
        P = len(T)
        o = _score_layout(P)

        def work(out, n_ptr, T_dev, s):
            if d2d:
                self._sources_for_batch(out, n_ptr, o["n_points"], s)
            self._score(T_dev, P, n_ptr, out.data_ptr() + o["score"] * 8, s, d2d)
        return PendingScores(P, *self._issue(rows, count, o["total"], o["n_points"] * 8, work, T))

    @torch.no_grad()
    def relocalise(self, rows, count, poses, keep: int = 8, with_normal: bool = False, iterations: int = None,
                   integrate: bool = False, max_cell_points: int = 0, carve: bool = False,
                   carve_options: dict = None, coarse_to_fine: bool = False, d2d: bool = False,
                   d2d_pyramid: bool = False) -> PendingRelocalisation:
        """Thin, score the P poses ``poses`` [P, 4, 4] (e.g. ``T_center @ pose_grid(...)``), keep the best ``keep`` (1..64)
        by (score descending, index ascending) among those with at least ``min_correspondences`` points counted, register
        from these as ``submit_batch`` does and select among the end poses as it selects.  Everything is issued on the
        current stream with no synchronisation in between; ``result()`` -> RelocalisationResult.  ``integrate`` and
        ``carve``: as for ``submit_batch``.  ``coarse_to_fine``: the grid is scored and its best ``keep`` chosen on the single
        map as ever; these are then registered as ``submit_batch(..., coarse_to_fine=True)`` registers them.
        ``d2d``: as for ``submit_batch``: the source cells are built once, the grid is scored as
        ``score_poses(..., d2d=True)`` scores it and its best ``keep`` are registered as ``submit_batch(..., d2d=True)``
        registers them.
        ``d2d_pyramid``: the grid is scored and its best ``keep`` chosen as ``score_poses(..., d2d=True)`` does it, with the
        single sources on the single map; these are then registered as ``submit_batch(..., d2d_pyramid=True)`` registers
        them."""
        def grid():
            T, K = _checked_poses(poses), int(keep)
            if not 1 <= K <= MAX_HYPOTHESES:
                raise ValueError(f"keep must be in [1, {MAX_HYPOTHESES}]")
            return T, K
        pyr = self._checked_d2d_pyramid("relocalise", d2d_pyramid, d2d, coarse_to_fine)
        if d2d:                                                      # the grid first: it needs no device
            self._checked_d2d("relocalise", d2d, coarse_to_fine)
        if d2d or pyr:
            grid()
        rows, copts = self._checked_for_batch("relocalise", rows, integrate, max_cell_points, carve, carve_options,
                                              coarse_to_fine, d2d, pyr)
        coarse_to_fine, d2d = coarse_to_fine or pyr, d2d or pyr
        T, K = grid()
        P = len(T)
        I = self.iterations if iterations is None else int(iterations)
        shape = self._batch_shape(integrate, carve, coarse_to_fine, d2d)
        so, o = _search_layout(P, K), _batch_layout(K, I, with_normal, *shape)

        def work(out, n_ptr, T_dev, s):
            sbase = out.data_ptr()
            if d2d:                                                  # the single sources: the grid is scored with them
                self._sources_for_batch(out, n_ptr, so["size"] + o["n_points"], s)
            if pyr:
                self._level_sources_for_batch(out, n_ptr, so["size"] + o["sources"], s)
            self._score(T_dev, P, n_ptr, sbase + so["score"] * 8, s, d2d)
            self.ctx.ndt_top_poses(sbase + so["score"] * 8, T_dev.data_ptr(), P, self.min_correspondences, K,
                                   sbase + so["top"] * 8, sbase + so["T_top"] * 8, sbase + so["n_top"] * 8, s)
            self._align_batch(n_ptr, sbase + so["T_top"] * 8, K, I, with_normal, sbase + so["size"] * 8, o, s, integrate,
                              max_cell_points, copts, coarse_to_fine, d2d)
        issued = self._issue(rows, count, so["size"] + o["total"], (so["size"] + o["n_points"]) * 8, work, T)
        return PendingRelocalisation(P, PendingPoses(K, I, with_normal, *issued, so["size"], *shape))

    def relocalise_filtered(self, pending, poses, **kw) -> PendingRelocalisation:
        """``relocalise`` of the kept rows of a pending SPSFilter / SPSCVMFilter frame, without the frame's result()."""
        return self.relocalise(pending._filtered, pending.count_dev, poses, **kw)

    def map_cells(self):
        """Debug: (keys uint64 [C], counts int32 [C], means [C, 3], inverse covariances [C, 6] as (xx, xy, xz, yy, yz, zz),
        valid bool [C]) of the device map, in ascending key order, as numpy arrays.  An online map gives its assigned
        cells in the order of their ids: the cells of the build in ascending key order, then the founded cells in the order
        they were founded."""
        return self._read_cells(None, self.n_cells, self.cell_capacity)

    def _read_cells(self, level, n_cells, capacity):
        """what ``map_cells`` gives, of the single map (``level`` None) or of a level of the pyramid: a static map
        (``capacity`` None) has ``n_cells`` cells, an online one room for ``capacity``, of which its info tells how many are
        assigned"""
        C = n_cells if capacity is None else capacity
        with torch.cuda.device(self.device):
            key = torch.zeros(C, dtype=torch.int64, device=self.device)
            cnt = torch.zeros(C, dtype=torch.int32, device=self.device)
            mean = torch.zeros((C, 3), dtype=torch.float64, device=self.device)
            icov = torch.zeros((C, 6), dtype=torch.float64, device=self.device)
            valid = torch.zeros(C, dtype=torch.int32, device=self.device)
            self.ctx._ndt_level_call("cells", level, key.data_ptr(), cnt.data_ptr(), mean.data_ptr(), icov.data_ptr(),
                                     valid.data_ptr())
        n = C if capacity is None else self.ctx._ndt_info(level)[0]
        return (key.cpu().numpy().view(np.uint64)[:n], cnt.cpu().numpy()[:n], mean.cpu().numpy()[:n], icov.cpu().numpy()[:n],
                valid.cpu().numpy().astype(bool)[:n])

    def pyramid_cells(self, level: int):
        """Debug: ``map_cells()`` of level ``level`` of the pyramid (0: the coarsest); an online pyramid gives the level's
        assigned cells in the order of their ids, as ``map_cells()`` does for an online map."""
        if self.resolutions is None:
            raise ValueError("pyramid_cells needs a localiser with resolutions")
        if not 0 <= int(level) < len(self.resolutions):
            raise ValueError(f"level must be in [0, {len(self.resolutions)})")
        caps = self.level_capacities
        return self._read_cells(int(level), self.level_cells[int(level)], None if caps is None else caps[int(level)])


@dataclass
class LoopStep:
    filter_result: object      # what the filter's result() returned
    pose_result: PoseResult
    guess: np.ndarray          # the pose the frame started from
    pose: np.ndarray           # the corrected pose handed on (the guess when flagged)
    flagged: bool              # the localiser reported status 2 or 3 (with hypotheses: none of them was selected), or lost
    batch: BatchPoseResult = None   # with hypotheses: every hypothesis of the frame (pose_result is the selected one's)
    search: RelocalisationResult = None   # a frame registered by the pose search (batch is then its candidates' batch)
    estimate: np.ndarray = None     # with an estimator: its pose after the frame's correction (None without one)
    match: MatchStatus = None       # the scan-matching status at the registered pose (a localiser with match_status)
    recovered: bool = False         # a ``recover`` frame whose global search found a pose that is not lost
    global_result: GlobalLocalisationResult = None   # a ``recover`` frame: what ``localise_global`` gave


class LocalisationLoop:
    """filter -> localiser -> pose back into the filter, one frame per ``step(scan)``:

      1. the guess: the loop's own constant-velocity prediction once its model holds four corrected poses, before that
         the last corrected pose, before that ``initial_pose`` (the loop's model holds corrected poses only: it starts
         without the leading identity of the node's list, so its first prediction averages three real motions);
      2. the filter: filters that take a pose get the guess, SPSCVMFilter predicts for itself as its node does,
         LTSFilter takes none;
      3. the localiser registers the filter's kept rows (sensor frame, as received) from the guess;
      4. the corrected pose goes to the loop's model and to the filter's ``add_pose`` where it has one; on status 2 or 3
         the guess is taken as the corrected pose and the step is flagged.

    One host synchronisation per frame where the filter's pending frame exposes its device rows (``_filtered`` and
    ``count_dev``: SPSFilter, SPSCVMFilter), two otherwise.

    ``hypotheses`` (NDTLocaliser only; None: one registration from the guess): offsets [K, 4, 4] with ``hypotheses[0]``
    the identity, e.g. from ``pose_grid``.  A frame is then registered from ``guess @ hypotheses[k]`` for every k at once
    (``submit_batch``) and the selected pose is handed on; a frame in which no hypothesis is selected (best = -1) is
    flagged and keeps the guess, as status 2 / 3 does without hypotheses.

    ``search`` (NDTLocaliser only; None: no pose search): offsets [P, 4, 4] (P <= 65536) with ``search[0]`` the identity.
    The first frame and every frame directly after a flagged frame are then registered by
    ``relocalise(guess @ search[k], keep=search_keep)`` instead of the plain or batch registration: the grid is scored, its
    best ``search_keep`` poses are aligned and the best end pose is handed on; a frame in which none is selected is flagged
    and keeps the guess.

    ``update_map`` (a localiser with an online map: ``NDTLocaliser(..., cell_capacity=N)``, or with an online pyramid:
    ``level_capacities``, whose frames report one result per level and take hypotheses and search with ``coarse_to_fine``
    only): every frame's kept points, as
    thinned for the registration, are folded into the map at the frame's corrected pose, behind the registration on its
    stream.  The device gates the update on the registration's status, so a flagged frame leaves the map alone; the
    frame's ``pose_result.map_update`` (``batch.map_update``) tells what happened.  ``max_cell_points``: the forgetting
    cap of ``NDTLocaliser.integrate``.

    ``carve_map`` (the same localisers): every frame's kept points are also cast as rays from the corrected pose and the
    map is carved (``NDTLocaliser.carve``; ``carve_options``: its keywords), under the same gate and before the update;
    the frame's ``pose_result.map_carve`` (``batch.map_carve``) tells what happened.

    ``estimator`` (a ``PoseEstimator``; None: everything above, unchanged): the guess of a frame is then the estimator's
    prediction -- ``step(scan, imu=rows)`` or ``step(scan, dt=seconds)`` say over what; frame 0 makes no prediction step
    and starts from the estimator's initial pose -- and the estimator's correction with the registered pose is queued
    behind the registration, gated on the device by its status as the map update and the carve are: a flagged frame keeps
    the guess and leaves the estimator uncorrected.  ``LoopStep.pose`` stays the registration's pose (where the map was
    updated and carved); ``LoopStep.estimate`` is the estimator's pose after the correction.  The loop's own
    constant-velocity model still receives the poses but is not asked.
    ``device_guess`` (None: where possible): the predicted pose starts the registration from the device
    (predict -> ``submit_from_device`` -> ``correct_from``, the guess read back with the frame's results: the one
    synchronisation per frame of the loop without an estimator).  That is possible where the filter takes no pose from the
    loop (SPSCVMFilter, LTSFilter, ``takes_pose`` false) and the localiser is an NDTLocaliser without hypotheses or search
    that registers points (``submit_from_device`` takes source cells with ``d2d`` only), and without a pyramid unless
    ``coarse_to_fine`` is set; the frame's ``batch`` is then the one-hypothesis batch.  Everywhere else, and with ``device_guess=False``, the
    predicted pose is fetched to the host first: one more small synchronisation per frame.  ``device_guess=True`` raises
    where the device path is impossible.

    ``coarse_to_fine`` (a localiser with ``resolutions``; False: everything above, unchanged): the frames of ``hypotheses``
    and ``search`` and the estimator's device path are registered on the pyramid (``submit_batch`` / ``relocalise`` /
    ``submit_from_device`` with ``coarse_to_fine=True``).  An online pyramid with ``update_map`` /
    ``carve_map`` may then take hypotheses and search, and with an estimator the device path is possible with a pyramid.

    ``d2d`` (a localiser with ``source="cells"``; False: everything above, unchanged, a cells localiser taking neither
    hypotheses nor search nor the device path): the frames of ``hypotheses`` and ``search`` and the estimator's device path
    are registered distribution to distribution (``submit_batch`` / ``relocalise`` / ``submit_from_device`` with
    ``d2d=True``).  Not with ``coarse_to_fine``.

    ``d2d_pyramid`` (a localiser with ``source="cells"`` and ``source_resolutions``; False: everything above, unchanged;
    not with ``d2d`` or ``coarse_to_fine``): the frames of ``hypotheses`` and ``search`` and the estimator's device path are
    registered distribution to distribution on the pyramid, as the plain ``submit`` of such a localiser registers
    (``submit_batch`` / ``relocalise`` / ``submit_from_device`` with ``d2d_pyramid=True``).  An online pyramid
    with ``update_map`` / ``carve_map`` may then take hypotheses and search, as with ``coarse_to_fine``.  ``recover`` stays
    refused as ever: a localiser with ``source="cells"`` has no ``global_grid``.

    A localiser with ``match_status``: a frame whose registration ends with status 0 or 1 but whose scan does
    not match the map at the registered pose (``match.lost``) is flagged as status 2 / 3 is: it keeps the guess, the map and
    the estimator stay untouched (the device gate, which is the status' verdict, already saw to that) and ``search`` frames
    follow as they do after any flagged frame.  ``LoopStep.match`` carries the status.

    ``recover`` (an NDTLocaliser with ``global_grid``; None: no recovery): ``dict(after=N, yaw_steps=A, keep=8,
    frontier=16384, min_score=1, scan_z=None, T_up=None)``, the last six the arguments of ``localise_global``.  After N >= 1
    flagged frames in a row the next frame is registered by ``localise_global`` instead of from the guess.  Where a pose is
    selected and not lost it is handed on, the loop's constant-velocity model is emptied (its motions would span the jump),
    an estimator is re-initialised at that pose (``PoseEstimator.reset``) and ``LoopStep.recovered`` is set; otherwise the
    frame is flagged and the count goes on, so the frame after it searches again.  ``LoopStep.global_result`` is what
    ``localise_global`` gave on such a frame (None on every other).  ``recover`` with ``device_guess=True`` is refused: a
    recovery frame reads the pose on the host anyway.  So is ``recover`` on an online pyramid with ``update_map`` or
    ``carve_map`` unless ``coarse_to_fine`` is set, as hypotheses and search are, and an estimator without ``reset``."""

    _RECOVER_DEFAULTS = dict(after=None, yaw_steps=None, keep=8, frontier=16384, min_score=1, scan_z=None, T_up=None)

    def __init__(self, filter, localiser, initial_pose, hypotheses=None, search=None, search_keep: int = 8,
                 update_map: bool = False, max_cell_points: int = 0, carve_map: bool = False, carve_options: dict = None,
                 estimator=None, device_guess=None, coarse_to_fine: bool = False, recover: dict = None, d2d: bool = False,
                 d2d_pyramid: bool = False):
        self.recover, self._flagged_run = None, 0
        if recover is not None:
            unknown = set(recover) - set(self._RECOVER_DEFAULTS)
            if unknown:
                raise ValueError(f"unknown recover entries {sorted(unknown)}")
            r = dict(self._RECOVER_DEFAULTS, **recover)
            if r["after"] is None or r["yaw_steps"] is None or int(r["after"]) < 1 or int(r["yaw_steps"]) < 1:
                raise ValueError("recover needs after >= 1 and yaw_steps >= 1")
            if getattr(localiser, "_global", None) is None or not hasattr(localiser, "localise_global"):
                raise ValueError("recover needs a localiser with an occupancy grid: NDTLocaliser(..., global_grid=dict(...))")
            if device_guess:
                raise ValueError("recover and device_guess=True exclude each other: a recovery frame reads the pose on the host")
            r["after"], r["yaw_steps"] = int(r["after"]), int(r["yaw_steps"])
            self.recover = r
        from .sps_filters import ConstantVelocityModel
        self.filter, self.localiser = filter, localiser
        # a localiser of the caller's own may have none of these: ScanToMapLocaliser's defaults then stand in
        source, caps, cell_capacity, resolutions = (getattr(localiser, a, getattr(ScanToMapLocaliser, a)) for a in
                                                    ("source", "level_capacities", "cell_capacity", "resolutions"))
        cells = source == "cells"
        self.d2d = bool(d2d)
        if self.d2d and not cells:
            raise ValueError("d2d=True needs an NDTLocaliser with source='cells'")
        if self.d2d and coarse_to_fine:
            raise ValueError("d2d=True and coarse_to_fine exclude each other: the pyramid registers points")
        self.d2d_pyramid = bool(d2d_pyramid)
        if self.d2d_pyramid and (self.d2d or coarse_to_fine):
            raise ValueError("d2d_pyramid=True excludes d2d and coarse_to_fine: it registers the scan's cells coarse to fine "
                             "by itself")
        if self.d2d_pyramid and (not cells or getattr(localiser, "source_resolutions", None) is None):
            raise ValueError("d2d_pyramid=True needs an NDTLocaliser with source='cells' and source_resolutions")
        if cells and not (self.d2d or self.d2d_pyramid) and (hypotheses is not None or search is not None):
            raise ValueError("hypotheses and search register points: they need an NDTLocaliser with source='points' "
                             "(or d2d=True, which registers the scan's cells)")
        self.coarse_to_fine = bool(coarse_to_fine)
        if self.coarse_to_fine and resolutions is None:
            raise ValueError("coarse_to_fine needs a localiser with a pyramid: NDTLocaliser(..., resolutions=...)")
        # what the batch, the search and the device path get on top of the keyword arguments below
        self._c2f = (dict(coarse_to_fine=True) if self.coarse_to_fine else dict(d2d=True) if self.d2d
                     else dict(d2d_pyramid=True) if self.d2d_pyramid else {})
        on_pyramid = self.coarse_to_fine or self.d2d_pyramid         # the batch, the search and the device path work there
        self.update_map, self.max_cell_points = bool(update_map), int(max_cell_points)
        online_pyramid = caps is not None
        if self.update_map and cell_capacity is None and not online_pyramid:
            raise ValueError("update_map needs a localiser with an online map: NDTLocaliser(..., cell_capacity=N)")
        if online_pyramid and (update_map or carve_map) and (hypotheses is not None or search is not None
                                                             or self.recover is not None) and not on_pyramid:
            raise ValueError("an online pyramid is updated and carved by the plain registration only: no hypotheses, no search, "
                             "no recover (unless coarse_to_fine)")
        # the keyword arguments every registration of the loop gets: none unless the map is updated
        self._kw = dict(integrate=True, max_cell_points=self.max_cell_points) if self.update_map else {}
        self.carve_map = bool(carve_map)
        if self.carve_map:
            if cell_capacity is None and not online_pyramid:
                raise ValueError("carve_map needs a localiser with an online map: NDTLocaliser(..., cell_capacity=N)")
            self._kw.update(carve=True, carve_options=carve_options)
        elif carve_options is not None:
            raise ValueError("carve_options needs carve_map=True")
        self.hypotheses = None
        self.search, self.search_keep, self._search_next = None, int(search_keep), True
        if search is not None:
            S = _checked_poses(search, what="search").copy()
            if not np.array_equal(S[0], np.eye(4)):
                raise ValueError("search[0] must be the identity")
            if not 1 <= self.search_keep <= MAX_HYPOTHESES:
                raise ValueError(f"search_keep must be in [1, {MAX_HYPOTHESES}]")
            if not hasattr(localiser, "relocalise"):
                raise TypeError("search needs a localiser with relocalise (NDTLocaliser)")
            self.search = S
        if hypotheses is not None:
            H = _checked_poses(hypotheses, "hypotheses", MAX_HYPOTHESES, "K").copy()
            if not np.array_equal(H[0], np.eye(4)):
                raise ValueError("hypotheses[0] must be the identity")
            if not hasattr(localiser, "submit_batch"):
                raise TypeError("hypotheses need a localiser with submit_batch (NDTLocaliser)")
            self.hypotheses = H
        self.estimator, self.device_guess = estimator, False
        if estimator is None:
            if device_guess:
                raise ValueError("device_guess needs an estimator")
        else:
            if not all(hasattr(estimator, a) for a in ("predict", "predict_imu", "pose_dev", "correct_from", "snapshot")):
                raise TypeError("estimator must be a PoseEstimator")
            if self.recover is not None and not hasattr(estimator, "reset"):
                raise TypeError("recover needs an estimator with reset (PoseEstimator): a recovered pose re-initialises it")
            takes_none = (hasattr(filter, "add_pose") or type(filter).__name__ == "LTSFilter"
                          or getattr(filter, "takes_pose", True) is False)
            possible = (takes_none and hasattr(localiser, "submit_from_device") and (resolutions is None or on_pyramid)
                        and hypotheses is None and search is None and (not cells or self.d2d or self.d2d_pyramid))
            if device_guess and not possible:
                raise ValueError("device_guess=True needs a filter that takes no pose from the loop and an NDTLocaliser without "
                                 "a pyramid, hypotheses or search")
            self.device_guess = (possible and self.recover is None) if device_guess is None else bool(device_guess)
        self._est_guess, self._est_wait, self._frames = None, None, 0
        self.initial_pose = np.array(_pose(initial_pose), dtype=np.float64)
        self.model = ConstantVelocityModel()
        self.model.poses = []                                        # corrected poses only
        self.poses = []                                              # the corrected pose of every frame

    def guess(self) -> np.ndarray:
        if self.estimator is not None:                               # the prediction step() fetched for this frame
            return self._est_guess.copy() if self._est_guess is not None else self.initial_pose.copy()
        if len(self.model.poses) >= 4:
            return self.model.predict()
        if self.model.poses:
            return self.model.poses[-1].copy()
        return self.initial_pose.copy()

    def _submit_filter(self, scan, guess):
        f = self.filter
        if hasattr(f, "add_pose"):                                   # SPSCVMFilter: the pose is its own prediction
            return f.submit(scan)
        if type(f).__name__ == "LTSFilter" or getattr(f, "takes_pose", True) is False:
            if not torch.is_tensor(scan):
                scan = torch.from_numpy(np.ascontiguousarray(np.asarray(scan)[:, :4], dtype=np.float32)).to(self.localiser.device)
            return f.submit(scan)
        return f.submit(scan, guess)

    def start_poses(self, guess) -> np.ndarray:
        """[K, 4, 4]: ``guess @ hypotheses[k]``"""
        return np.stack([guess @ h for h in self.hypotheses])

    def search_poses(self, guess) -> np.ndarray:
        """[P, 4, 4]: ``guess @ search[k]``"""
        return np.stack([guess @ d for d in self.search])

    def _queue_correction(self, pose_pend, correct=True):
        """with an estimator: its correction behind the registration just issued, then a copy of its state for the host.  A
        recovery frame queues no correction (``correct`` false): its pose re-initialises the estimator, or is not handed on"""
        if self.estimator is not None:
            if correct:
                self.estimator.correct_from(pose_pend)
            self._est_wait = self.estimator.snapshot()

    def _predict(self, imu, dt):
        """the estimator's prediction for this frame, queued; frame 0 makes no step"""
        est = self.estimator
        if self._frames == 0 or (imu is not None and len(imu) == 0):
            est.predict_imu(np.zeros((0, 7)))
        elif imu is not None:
            est.predict_imu(imu)
        elif dt is not None:
            est.predict(dt)
        else:
            raise ValueError("with an estimator every frame after the first needs imu=rows or dt=seconds")
        self._frames += 1

    def step(self, scan, imu=None, dt=None) -> LoopStep:
        if self.estimator is None:
            if imu is not None or dt is not None:
                raise ValueError("imu and dt need an estimator")
        else:
            self._predict(imu, dt)
            if self.device_guess:                                    # predict -> filter -> submit_from_device(pose_dev) -> correct_from
                return self._register(scan, None, "submit_from_device", (self.estimator.pose_dev,), self._c2f, self._read_batch)
            self._est_guess = self.estimator.pose_dev.cpu().numpy().astype(np.float64)   # the one more synchronisation
        guess = self.guess()
        if self.recover is not None and self._flagged_run >= self.recover["after"]:
            r = self.recover
            kw = dict(self._c2f, **{k: r[k] for k in ("keep", "frontier", "min_score", "scan_z", "T_up")})
            out = self._register(scan, guess, "localise_global", (r["yaw_steps"],), kw, self._read_global, recovering=True)
        elif self.search is not None and self._search_next:
            out = self._register(scan, guess, "relocalise", (self.search_poses(guess),), dict(self._c2f, keep=self.search_keep),
                                 self._read_search)
        elif self.hypotheses is not None:
            out = self._register(scan, guess, "submit_batch", (self.start_poses(guess),), self._c2f, self._read_batch)
        else:
            out = self._register(scan, guess, "submit", (guess,), {}, self._read_pose)
        self._search_next = out.flagged
        return out

    # how a registration's result reads: -> (flagged, the pose it hands on, PoseResult, BatchPoseResult, RelocalisationResult,
    # MatchStatus or None); a result of the caller's own localiser may have no ``match``
    @staticmethod
    def _lost(match):
        return match is not None and bool(match.lost)

    @classmethod
    def _read_pose(cls, pres):
        m = getattr(pres, "match", None)
        return pres.status in (FEW_CORRESPONDENCES, SINGULAR) or cls._lost(m), pres.pose, pres, None, None, m

    @classmethod
    def _read_batch(cls, bres):
        m = getattr(bres, "match", None)
        return bres.best < 0 or cls._lost(m), bres.pose, bres.results[max(bres.best, 0)], bres, None, m

    @classmethod
    def _read_search(cls, sres):
        m = getattr(sres.batch, "match", None)
        return sres.index < 0 or cls._lost(m), sres.pose, sres.batch.results[max(sres.batch.best, 0)], sres.batch, sres, m

    @classmethod
    def _read_global(cls, gres):
        m = getattr(gres.batch, "match", None)
        return gres.index < 0 or cls._lost(m), gres.pose, gres.batch.results[max(gres.batch.best, 0)], gres.batch, None, m

    # the localiser's entry points that take a filter's pending frame in place of (rows, count)
    _FILTERED = dict(submit="submit_filtered", submit_batch="submit_filtered_batch", relocalise="relocalise_filtered",
                     localise_global="localise_global_filtered")

    def _register(self, scan, guess, method, args, kw, read, recovering=False) -> LoopStep:
        """One frame through the filter and ``localiser.<method>(rows, count, *args, **kw)``; ``read`` (above) reads its
        result.  Where the filter's pending frame exposes its device rows, the registration and the estimator's correction
        are queued before the filter's ``result()``, so nothing synchronises between filter and localiser; otherwise they
        follow it.  ``guess`` None: the registration starts from the estimator's device pose, and the guess comes back with
        the estimator's snapshot, which is waited on last."""
        pend = self._submit_filter(scan, guess)
        kw = dict(kw, **self._kw)
        if hasattr(pend, "count_dev") and hasattr(pend, "_filtered"):
            if method in self._FILTERED:
                pose_pend = getattr(self.localiser, self._FILTERED[method])(pend, *args, **kw)
            else:
                pose_pend = getattr(self.localiser, method)(pend._filtered, pend.count_dev, *args, **kw)
            self._queue_correction(pose_pend, not recovering)
            fres = pend.result()
        else:
            fres = pend.result()
            kept = fres.filtered
            pose_pend = getattr(self.localiser, method)(kept, len(kept), *args, **kw)
            self._queue_correction(pose_pend, not recovering)
        res = pose_pend.result()
        flagged, pose, pres, bres, sres, match = read(res)
        estimate = None
        if self.estimator is not None:
            wait, self._est_wait = self._est_wait, None
            state, predicted = wait()
            estimate, guess = state.pose, predicted if guess is None else guess
        recovered = recovering and not flagged
        if recovered:                                                # the model's motions span the jump
            self.model.poses = []
            if self.estimator is not None:
                self.estimator.reset(pose)
                estimate = np.array(pose, dtype=np.float64)
        self._flagged_run = self._flagged_run + 1 if flagged else 0
        self._hand_on(guess if flagged else pose)
        return LoopStep(fres, pres, guess, self.poses[-1], flagged, bres, sres, estimate, match, recovered,
                        res if recovering else None)

    def _hand_on(self, pose):
        """the frame's corrected pose to the loop's model, to the filter's ``add_pose`` where it has one, and to ``poses``"""
        self.model.add_pose(pose)
        if hasattr(self.filter, "add_pose"):
            self.filter.add_pose(pose)
        self.poses.append(np.array(pose, dtype=np.float64))
