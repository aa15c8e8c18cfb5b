#!/usr/bin/env python3
"""Per-frame cost of the scan-to-map localiser on one MI355X at config-2 size (64 x 1750 rays, ~100 k points, the
synthetic.build_map() map, max_distance 1 m, leaf 0.2 m):

  localiser   sps_loc_downsample + sps_loc_align of a whole scan, 0.2 m / 1 degree off its true pose, timed with
              hipEvents around submit() over --frames frames after --warmup; the iteration count beside it
  restatement the numpy restatement (tests/localiser_reference.py) on --cpu-frames of the same frames: a stated
              baseline, not a target
  loop        LocalisationLoop.step() with SPSCVMFilter (host wall clock, one synchronisation per frame) beside
              SPSFilter alone on the same scans

    python tools/localiser_timing.py [--frames 200] [--warmup 20] [--cpu-frames 1] [--one-frame] [--cpu-only]
                                     [--localiser {icp,ndt}] [--hypotheses K] [--search P] [--update-map] [--carve]
                                     [--source {points,cells}] [--source-resolution R] [--source-min-points N] [--global]
                                     [--d2d] [--source-resolutions S0,S1,...] [--start-behind M] [--d2d-pyramid]

``--localiser ndt`` times sps_amd.localiser.NDTLocaliser (1 m cells, 7 neighbours) on the same frames and from the same
start, prints the ICP's per-frame figures of the same session beside it and the build time of both maps; the
restatement is then tests/ndt_reference.py.

``--localiser ndt --hypotheses K`` times NDTLocaliser.submit_batch from K start poses (the guess and offsets 0.5 m apart
around it) against K back-to-back submit calls from the same poses, and against one submit.

``--localiser ndt --search P`` times NDTLocaliser.score_poses of P poses against ceil(P / 64) calls of
submit_batch(iterations=0) over the same poses and checks that the two agree bit for bit.

``--localiser ndt --resolutions 2,1,0.5`` times the coarse-to-fine pyramid (NDTLocaliser(..., resolutions=...)) beside the
single-map localiser on the same frames in one session: per-frame time, live and idle slots, and the map builds.

``--localiser ndt --update-map`` times the online map (NDTLocaliser(..., cell_capacity=N)): sps_ndt_map_update alone and
submit(integrate=True) against submit, interleaved frame by frame with the only alternative a static map offers, a new
NDTLocaliser over map + frame.

``--localiser ndt --resolutions 2,1,0.5 --integrate --carve`` times the online pyramid (NDTLocaliser(..., level_capacities=...)):
sps_ndt_pyramid_update and sps_ndt_pyramid_carve against one sps_ndt_map_update / sps_ndt_map_carve per level on single-map
localisers of the same resolutions and capacities, frame by frame alternating in one run, and submit(integrate=True,
carve=True) against the pyramid's plain submit.

``--localiser ndt --carve`` times the free-space carving of the online map: sps_ndt_map_carve alone, sps_ndt_map_update alone,
submit and submit(integrate=True, carve=True), interleaved frame by frame, and (with --cpu-frames >= 1) the restatement's
count of the cells a ray visits on one frame.

``--localiser ndt --estimator`` times the pose estimator (sps_amd.pose_estimator.PoseEstimator) beside the registration:
sps_ukf_predict over M = 1, 10 and 40 IMU rows already on the device, predict_imu of the same rows (with their pinned
upload), the IMU-less step and the correction (hipEvents around each, a prediction and a correction alternating so the
state stays that of a running filter); then LocalisationLoop(SPSCVMFilter, NDTLocaliser) per frame (host wall clock)
without an estimator, with one on the device path and with one on the host path, the three alternating frame by frame.

``--localiser ndt --source cells`` times distribution-to-distribution registration (NDTLocaliser(..., source="cells")):
per frame the hipEvent time around submit(), the iterations, the scan's valid source cells and the error against the true
pose, beside the point path on the same frames, the two alternating frame by frame in one run; then the source build alone
and the loop with each.

``--localiser ndt --source cells --resolutions 2,1,0.5 --source-resolutions 2,1,0.5`` times the coarse-to-fine registration
of the scan's cells (NDTLocaliser(..., source_resolutions=...)) beside the single cells localiser and the
point pyramid, frame by frame alternating in one run, with the live slots per level, and the source build of all levels
in one call against one single build per level; ``--start-behind 0.5`` starts that far behind the usual start pose.

``--localiser ndt --source cells --d2d`` with any of ``--search P``, ``--hypotheses K``, ``--estimator`` times the
distribution-to-distribution calls that take several poses beside the point path's on the same frames, the two
alternating frame by frame, hipEvents around each call: score_poses of P poses and relocalise(keep=8) over them; submit_batch
from K start poses; and LocalisationLoop(SPSCVMFilter, ., ukf) per frame (host wall clock) on cells with ``d2d`` (device
path), on cells without (the guess fetched) and on points (device path).  With --one-frame and --search: a warm-up and ONE
score_poses on each path, the target of a kernel trace.

``--localiser ndt --source cells --resolutions R0,R1,... --source-resolutions S0,S1,... --d2d-pyramid`` times the batched
coarse-to-fine registration of the scan's cells, hipEvents around each call, the sides of one table alternating
frame by frame with the order swapped every frame: submit_batch(d2d_pyramid=True) for K = 8 and 64 against K back-to-back
submit calls on the same localiser and against the point pyramid's submit_batch(coarse_to_fine=True); with ``--search P``
relocalise(d2d_pyramid=True) over P poses against the point pyramid's; then LocalisationLoop(SPSCVMFilter, ., ukf) per frame
(host wall clock) with ``d2d_pyramid`` on the device path against the host path of the same localiser.

``--localiser ndt --resolutions R0,R1,... --coarse-to-fine`` times the batched coarse-to-fine registration,
hipEvents around each call and the calls of one table alternating frame by frame: submit_from_device(coarse_to_fine=True)
against submit on the pyramid (K = 1); submit_batch(coarse_to_fine=True) against the single-map submit_batch for K = 8 and
64 at the budgets 30 (caps 10 each) and 90 (caps 30 each); then LocalisationLoop per frame (host wall clock) with the UKF
on the pyramid, device path against host path, and the same loop on an online pyramid with update and carve.

``--localiser ndt --global`` times the global search on the synthetic map with the slice of
scripts/filter_sequence.py --global-start (0.5 m cells, map and scan slice -1 .. 3 m, 72 yaws, 3 levels, frontier 16384):
hipEvents around global_search and around localise_global (keep 8), the two alternating frame by frame, the scan moved to
a pose the search has to find; then, on --cpu-frames frames, the only comparable means without it: score_poses over the
poses of all leaves in chunks of 65536 (the pose upload included), and whether its best leaf is the search's.  With
--one-frame: a warm-up and ONE global_search.

``--match-status`` (either localiser): hipEvents around ``submit`` of a localiser without and one with ``match_status``
(max_distance 0.5; the ICP's grid has 1 m cells, the NDT localiser's own 0.5 m), the two alternating frame by frame, and around
the status' two launches alone at the pose and on the thinned points the last frame left.

``--one-frame`` runs a warm-up and ONE localiser frame: the target of a ``rocprofv3 --kernel-trace --stats`` run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import sps_oracle as O  # noqa: E402
from sps_amd import synthetic  # noqa: E402
from sps_amd.localiser import LocalisationLoop, NDTLocaliser, ScanToMapLocaliser  # noqa: E402
from sps_amd.sps_filters import SPSCVMFilter, SPSFilter  # noqa: E402
from tests import localiser_reference as LR  # noqa: E402
from tests import ndt_reference as NR  # noqa: E402
from tests.helpers import CFG, net_from_params  # noqa: E402

VS, EPS = CFG["MODEL"]["VOXEL_SIZE"], CFG["FILTER"]["THRESHOLD"]


def timed_frames(loc, dscans, T_init, warmup, frames):
    """hipEvent time around submit() per frame -> (ms, iterations, points, errors against the true pose I)"""
    st = torch.cuda.current_stream()
    ms, iters, npts, errs = [], [], [], []
    for k in range(warmup + frames):
        s = dscans[k % len(dscans)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        pend = loc.submit(s, len(s), T_init)
        e1.record(st)
        r = pend.result()
        e1.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
            iters.append(r.iterations)
            npts.append(r.n_points)
            errs.append(LR.pose_difference(r.pose, np.eye(4))[0])
    return ms, iters, npts, errs


def match_status_main(a, dscans, mp, T_init):
    """submit without and with match_status, alternating frame by frame; then the status' two launches alone"""
    from sps_amd.localiser import MATCH_WORDS
    make = (lambda **kw: NDTLocaliser(mp[:, :3], **kw)) if a.localiser == "ndt" else (lambda **kw: ScanToMapLocaliser(mp[:, :3], **kw))
    locs = {"without": make(), "with": make(match_status=dict(min_inlier_fraction=0.5))}
    st = torch.cuda.current_stream()
    ms = {k: [] for k in locs}
    frac, lost = [], 0
    for k in range(a.warmup + a.frames):
        s = dscans[k % len(dscans)]
        for name in (("without", "with") if k % 2 == 0 else ("with", "without")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            pend = locs[name].submit(s, len(s), T_init)
            e1.record(st)
            r = pend.result()
            e1.synchronize()
            if k >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
                if name == "with":
                    frac.append(r.match.inlier_fraction)
                    lost += bool(r.match.lost)
    loc = locs["with"]
    out_words = torch.zeros(MATCH_WORDS + 1, dtype=torch.float64, device="cuda")
    out_words[MATCH_WORDS:].view(torch.int32)[0] = r.n_points
    T_dev = torch.from_numpy(np.ascontiguousarray(r.pose)).cuda()
    alone = []
    for k in range(a.warmup + a.frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        loc._status(out_words.data_ptr() + MATCH_WORDS * 8, T_dev.data_ptr(), None, out_words.data_ptr(), st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        if k >= a.warmup:
            alone.append(e0.elapsed_time(e1))
    med = lambda v: round(float(np.median(v)), 4)
    out = {"localiser": a.localiser, "frames": a.frames, "warmup": a.warmup, "points_after_thinning": int(r.n_points),
           "submit_ms": {k: {"median": med(v), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()},
           "submit_difference_ms": round(med(ms["with"]) - med(ms["without"]), 4),
           "status_alone_ms": {"median": med(alone), "min": round(min(alone), 4), "max": round(max(alone), 4)},
           "inlier_fraction_min": round(min(frac), 4), "lost": lost}
    print(f"submit without match_status median {out['submit_ms']['without']['median']:.3f} ms, with {out['submit_ms']['with']['median']:.3f} ms; "
          f"the status' two launches alone median {out['status_alone_ms']['median']:.4f} ms on {out['points_after_thinning']} points",
          flush=True)
    print(json.dumps(out))


def build_ms(make):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loc = make()
    torch.cuda.synchronize()
    return loc, (time.perf_counter() - t0) * 1e3


def restatement_only(a):
    mp = synthetic.build_map()
    T_init = LR.perturbation(0.15, 0.12, 0.05, 1.0)
    if a.localiser == "ndt":
        cmap = NR.cells(mp[:, :3].astype(np.float64), 1.0)
        for k in range(max(a.cpu_frames, 1)):
            s = synthetic.lidar_scan(seed=40 + (a.warmup + k) % 12, n_beams=64, n_azimuth=1750)
            t0 = time.perf_counter()
            _, pts = LR.downsample(s, len(s), 0.2, 1 << 16)
            r = NR.align(pts, cmap, T_init)
            print(f"NDT restatement frame {k}: {time.perf_counter() - t0:.1f} s, {len(pts)} points, {r['iterations']} iterations, "
                  f"status {r['status']}", flush=True)
        return
    index = LR.MapIndex(mp, 1.0)
    for k in range(max(a.cpu_frames, 1)):
        s = synthetic.lidar_scan(seed=40 + (a.warmup + k) % 12, n_beams=64, n_azimuth=1750)
        t0 = time.perf_counter()
        _, pts = LR.downsample(s, len(s), 0.2, 1 << 16)
        r = LR.align(pts, index, T_init, 30, 50, 1e-4, 1e-5)
        print(f"restatement frame {k}: {time.perf_counter() - t0:.1f} s, {len(pts)} points, {r['iterations']} iterations, "
              f"status {r['status']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cpu-frames", type=int, default=1)
    ap.add_argument("--one-frame", action="store_true")
    ap.add_argument("--cpu-only", action="store_true", help="only the restatement's CPU time (needs no GPU)")
    ap.add_argument("--localiser", choices=("icp", "ndt"), default="icp")
    ap.add_argument("--hypotheses", type=int, default=0, help="with --localiser ndt: time submit_batch of K start poses "
                    "against K back-to-back submit calls")
    ap.add_argument("--search", type=int, default=0, help="with --localiser ndt: time score_poses of P poses against "
                    "ceil(P / 64) submit_batch(iterations=0) calls, the only way to score poses without it")
    ap.add_argument("--update-map", "--integrate", dest="update_map", action="store_true", help="with --localiser ndt: time the online map's update against "
                    "rebuilding the localiser over map + frame")
    ap.add_argument("--carve", action="store_true", help="with --localiser ndt: time the online map's free-space carving beside "
                    "its update and the registration")
    ap.add_argument("--resolutions", type=str, default=None, help="with --localiser ndt: R0,R1,... time the coarse-to-fine "
                    "pyramid beside the single-map localiser, in the same session")
    ap.add_argument("--iterations", type=int, default=30, help="with --resolutions: the pyramid's budget of slots")
    ap.add_argument("--level-iterations", type=str, default=None, help="with --resolutions: N0,N1,... the cap of every level")
    ap.add_argument("--coarse-to-fine", dest="c2f", action="store_true", help="with --resolutions: time the batched "
                    "coarse-to-fine registration against the calls it extends")
    ap.add_argument("--estimator", action="store_true", help="with --localiser ndt: time the UKF pose estimator's calls and the "
                    "loop with it, on the device path and the host path")
    ap.add_argument("--source", choices=("points", "cells"), default="points", help="with --localiser ndt: cells times "
                    "distribution-to-distribution registration beside the point path")
    ap.add_argument("--source-resolution", type=float, default=None, help="with --source cells: edge of the scan's cells")
    ap.add_argument("--source-min-points", type=str, default=None, help="with --source cells: points a cell of the scan needs; "
                    "with --source-resolutions also N0,N1,..., one per level")
    ap.add_argument("--source-resolutions", type=str, default=None, help="with --source cells --resolutions R0,R1,...: S0,S1,... "
                    "time the coarse-to-fine registration of the scan's cells beside the single cells localiser and the point "
                    "pyramid")
    ap.add_argument("--start-behind", type=float, default=0.0, help="with --source-resolutions: start this many metres behind "
                    "the usual start pose, along x")
    ap.add_argument("--d2d", action="store_true", help="with --source cells and any of --search, --hypotheses, --estimator: time "
                    "the d2d=True calls beside the point path's")
    ap.add_argument("--d2d-pyramid", dest="d2d_pyramid", action="store_true", help="with --source cells --resolutions "
                    "--source-resolutions: time the d2d_pyramid=True calls beside K submits and the point pyramid's batch")
    ap.add_argument("--match-status", dest="match_status", action="store_true", help="time submit without and with the "
                    "scan-matching status, alternating, and the status' two launches alone")
    ap.add_argument("--global", dest="global_search", action="store_true", help="with --localiser ndt: time global_search and "
                    "localise_global against score_poses over all leaf poses")
    a = ap.parse_args()
    if a.global_search and (a.localiser != "ndt" or a.hypotheses or a.search or a.update_map or a.carve or a.resolutions
                            or a.estimator or a.source == "cells"):
        ap.error("--global needs --localiser ndt and none of the other modes")
    if a.d2d and (a.source != "cells" or a.localiser != "ndt" or not (a.hypotheses or a.search or a.estimator) or a.update_map
                  or a.carve or a.resolutions or a.global_search or a.match_status):
        ap.error("--d2d needs --localiser ndt --source cells, any of --search, --hypotheses, --estimator, and no other mode")
    try:
        if a.source_min_points is not None:
            mps = tuple(int(v) for v in a.source_min_points.split(","))
            a.source_min_points = mps[0] if len(mps) == 1 else mps
        if a.source_resolutions is not None:
            a.source_resolutions = tuple(float(v) for v in a.source_resolutions.split(","))
    except ValueError:
        ap.error("--source-min-points takes integers and --source-resolutions numbers, separated by commas")
    if a.d2d_pyramid and (a.localiser != "ndt" or a.source != "cells" or not a.resolutions or a.source_resolutions is None
                          or a.d2d or a.c2f or a.hypotheses or a.update_map or a.carve or a.estimator or a.one_frame
                          or a.source_resolution is not None):
        ap.error("--d2d-pyramid needs --localiser ndt --source cells --resolutions --source-resolutions and, of the other modes, "
                 "at most --search")
    if a.source_resolutions is not None and (a.localiser != "ndt" or a.source != "cells" or not a.resolutions or a.d2d or a.c2f
                                             or a.hypotheses or (a.search and not a.d2d_pyramid) or a.update_map or a.carve
                                             or a.estimator or a.source_resolution is not None):
        ap.error("--source-resolutions needs --localiser ndt --source cells --resolutions and none of the other modes")
    if isinstance(a.source_min_points, tuple) and a.source_resolutions is None:
        ap.error("a --source-min-points list needs --source-resolutions")
    if a.source == "cells" and not a.d2d and (a.localiser != "ndt" or a.hypotheses or (a.search and not a.d2d_pyramid)
                                              or a.update_map or a.carve
                                              or (a.resolutions and a.source_resolutions is None) or a.estimator):
        ap.error("--source cells needs --localiser ndt and none of the other modes (--d2d: with --search, --hypotheses, --estimator)")
    if (a.source_resolution is not None or a.source_min_points is not None) and a.source != "cells":
        ap.error("--source-resolution and --source-min-points need --source cells")
    if a.estimator and not a.d2d and (a.localiser != "ndt" or a.hypotheses or a.search or a.update_map or a.carve or a.resolutions):
        ap.error("--estimator needs --localiser ndt and none of the other modes")
    if a.c2f and (not a.resolutions or a.update_map or a.carve or a.estimator or a.one_frame):
        ap.error("--coarse-to-fine needs --resolutions and none of --update-map, --carve, --estimator, --one-frame")
    if a.resolutions and (a.localiser != "ndt" or a.hypotheses or (a.search and not a.d2d_pyramid)):
        ap.error("--resolutions needs --localiser ndt and none of --hypotheses, --search")
    if a.carve and (a.localiser != "ndt" or a.hypotheses or a.search or (a.update_map and not a.resolutions)):
        ap.error("--carve needs --localiser ndt and none of --hypotheses, --search, --update-map (but with --resolutions)")
    if a.update_map and a.localiser != "ndt":
        ap.error("--update-map needs --localiser ndt")
    if a.search and (a.localiser != "ndt" or not 1 <= a.search <= 65536):
        ap.error("--search P needs --localiser ndt and 1 <= P <= 65536")
    if a.hypotheses and (a.localiser != "ndt" or not 1 <= a.hypotheses <= 64):
        ap.error("--hypotheses K needs --localiser ndt and 1 <= K <= 64")
    if a.cpu_only:
        return restatement_only(a)
    assert torch.cuda.is_available(), "localiser_timing needs the MI355X"
    scans = [synthetic.lidar_scan(seed=40 + i, n_beams=64, n_azimuth=1750) for i in range(12)]   # world frame = sensor at I
    dscans = [torch.from_numpy(s).cuda() for s in scans]
    mp = synthetic.build_map()
    T_init = LR.perturbation(0.15, 0.12, 0.05, 1.0)
    if a.match_status:
        return match_status_main(a, dscans, mp, T_init)
    if a.global_search:
        return ndt_global_main(a, scans, mp)
    if a.d2d:
        return ndt_d2d_batch_main(a, scans, dscans, mp, T_init)
    if a.estimator:
        return ndt_estimator_main(a, scans, dscans, mp, T_init)
    if a.c2f:
        return ndt_c2f_main(a, scans, dscans, mp, T_init)
    if a.d2d_pyramid:
        return ndt_d2d_pyramid_batch_main(a, scans, dscans, mp, T_init)
    if a.source_resolutions is not None:
        return ndt_d2d_pyramid_main(a, scans, dscans, mp, T_init)
    if a.localiser == "ndt" and a.resolutions and (a.update_map or a.carve):
        return ndt_online_pyramid_main(a, dscans, mp, T_init)
    if a.localiser == "ndt" and a.update_map:
        return ndt_update_main(a, dscans, mp, T_init)
    if a.localiser == "ndt" and a.carve:
        return ndt_carve_main(a, scans, dscans, mp, T_init)
    if a.localiser == "ndt" and a.search:
        return ndt_search_main(a, dscans, mp, T_init)
    if a.localiser == "ndt" and a.hypotheses:
        return ndt_batch_main(a, dscans, mp, T_init)
    if a.localiser == "ndt" and a.resolutions:
        return ndt_pyramid_main(a, dscans, mp, T_init)
    if a.localiser == "ndt" and a.source == "cells":
        return ndt_d2d_main(a, scans, dscans, mp, T_init)
    if a.localiser == "ndt":
        return ndt_main(a, scans, dscans, mp, T_init)
    loc = ScanToMapLocaliser(mp[:, :3])

    def frame(k):
        s = dscans[k % len(dscans)]
        return loc.submit(s, len(s), T_init)

    for k in range(a.warmup):
        frame(k).result()
    torch.cuda.synchronize()
    if a.one_frame:
        r = frame(a.warmup).result()
        print(json.dumps({"one_frame": True, "status": r.status, "iterations": r.iterations, "n_points": r.n_points}))
        return
    st = torch.cuda.current_stream()
    ms, iters, npts, errs = [], [], [], []
    for k in range(a.frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        pend = frame(a.warmup + k)
        e1.record(st)
        r = pend.result()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        iters.append(r.iterations)
        npts.append(r.n_points)
        errs.append(LR.pose_difference(r.pose, np.eye(4))[0])
    out = {"n_scan": int(np.mean([len(s) for s in scans])), "n_map": len(mp), "frames": a.frames, "warmup": a.warmup,
           "localiser_ms": {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)},
           "iterations": {"median": float(np.median(iters)), "min": min(iters), "max": max(iters)},
           "points_after_thinning": int(np.mean(npts)), "max_error_m": round(max(errs), 5)}
    out["ms_per_iteration"] = round(out["localiser_ms"]["median"] / max(out["iterations"]["median"], 1), 4)
    print(f"localiser  median {out['localiser_ms']['median']:.3f} ms (min {min(ms):.3f} max {max(ms):.3f}) per frame, "
          f"iterations median {out['iterations']['median']:.0f}, {out['points_after_thinning']} points after thinning", flush=True)

    cpu = []
    index = LR.MapIndex(mp, loc.max_distance) if a.cpu_frames else None
    for k in range(a.cpu_frames):
        s = scans[(a.warmup + k) % len(scans)]
        t0 = time.perf_counter()
        _, pts = LR.downsample(s, len(s), loc.leaf, loc.capacity)
        r = LR.align(pts, index, T_init, loc.iterations, loc.min_correspondences, loc.tol_t, loc.tol_r)
        cpu.append(time.perf_counter() - t0)
        print(f"restatement frame {k}: {cpu[-1]:.1f} s, {r['iterations']} iterations, status {r['status']}", flush=True)
    if cpu:
        out["restatement_s"] = round(float(np.median(cpu)), 2)

    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(mp)
    sps = SPSFilter(net, mpt, voxel_size=VS, epsilon=EPS)
    cvm = SPSCVMFilter(net, mpt, voxel_size=VS, epsilon=EPS)
    loop = LocalisationLoop(cvm, loc, np.eye(4))
    t_sps, t_loop, flagged = [], [], 0
    for k in range(a.warmup + a.frames):
        s = scans[k % len(scans)]
        t0 = time.perf_counter()
        sps(s, np.eye(4))
        t1 = time.perf_counter()
        step = loop.step(s)
        t2 = time.perf_counter()
        if k >= a.warmup:
            t_sps.append(t1 - t0)
            t_loop.append(t2 - t1)
            flagged += step.flagged
    out["sps_filter_ms"] = round(float(np.median(t_sps)) * 1e3, 4)
    out["loop_sps_cvm_ms"] = round(float(np.median(t_loop)) * 1e3, 4)
    out["loop_flagged_frames"] = int(flagged)
    print(f"SPSFilter alone {out['sps_filter_ms']:.3f} ms, LocalisationLoop(sps_cvm) {out['loop_sps_cvm_ms']:.3f} ms per frame "
          f"({flagged} flagged)")
    print(json.dumps(out))


GLOBAL = dict(grid=dict(resolution=0.5, map_z=(-1.0, 3.0), levels=3), scan_z=(-1.0, 3.0), yaw_steps=72, frontier=16384, keep=8)


def ndt_global_main(a, scans, mp):
    """--global: see the module docstring.  The scans are taken at the identity; they are moved into the sensor frame of
    T_true, so the search has a pose to find that is not the origin of the grid"""
    th = np.radians(40.0)
    T_true = np.eye(4)
    T_true[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    T_true[:2, 3] = [2.3, 0.4]
    Ti = np.linalg.inv(T_true)
    moved = [np.c_[s[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3], s[:, 3]].astype(np.float32) for s in scans]
    dscans = [torch.from_numpy(s).cuda() for s in moved]
    loc, t_build = build_ms(lambda: NDTLocaliser(mp[:, :3], global_grid=GLOBAL["grid"]))
    g, A, kw = loc._global, GLOBAL["yaw_steps"], dict(keep=GLOBAL["keep"], frontier=GLOBAL["frontier"], scan_z=GLOBAL["scan_z"])
    st = torch.cuda.current_stream()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        pend = call()
        e1.record(st)
        r = pend.result() if hasattr(pend, "result") else pend
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for k in range(a.warmup):
        s = dscans[k % len(dscans)]
        loc.global_search(s, len(s), A, **kw).result()
        loc.localise_global(s, len(s), A, **kw).result()
    torch.cuda.synchronize()
    if a.one_frame:
        s = dscans[a.warmup % len(dscans)]
        r = loc.global_search(s, len(s), A, **kw).result()
        print(json.dumps({"one_frame": True, "n_found": r.n_found, "certified": r.certified, "n_slice": r.n_slice}))
        return
    ms_s, ms_l, cert, err_leaf, err_pose, ok, cands = [], [], [], [], [], 0, []
    for k in range(a.frames):
        s = dscans[(a.warmup + k) % len(dscans)]
        t, r = timed(lambda: loc.global_search(s, len(s), A, **kw))
        ms_s.append(t)
        cert.append(r.certified)
        cands.append(int(r.candidates.sum()))
        err_leaf.append(float(np.linalg.norm(r.poses[0][:2, 3] - T_true[:2, 3])))
        t, r2 = timed(lambda: loc.localise_global(s, len(s), A, **kw))
        ms_l.append(t)
        ok += r2.ok
        err_pose.append(LR.pose_difference(r2.pose, T_true)[0])
    med = lambda v: round(float(np.median(v)), 4)
    out = {"n_scan": int(np.mean([len(s) for s in scans])), "n_map": len(mp), "frames": a.frames, "warmup": a.warmup,
           "grid": [g["W"], g["H"]], "leaves": A * g["W"] * g["H"], "settings": {k: v for k, v in GLOBAL.items() if k != "grid"},
           "grid_settings": GLOBAL["grid"], "build_ms": round(t_build, 2),
           "global_search_ms": {"median": med(ms_s), "min": round(min(ms_s), 4), "max": round(max(ms_s), 4)},
           "localise_global_ms": {"median": med(ms_l), "min": round(min(ms_l), 4), "max": round(max(ms_l), 4)},
           "certified_min": int(min(cert)), "nodes_scored_median": med(cands), "best_leaf_error_m_max": round(max(err_leaf), 4),
           "localise_global_selected": int(ok), "localise_global_error_m_max": round(max(err_pose), 5),
           "points_after_thinning": r.n_points, "points_in_slice": r.n_slice}
    print(f"global_search  median {out['global_search_ms']['median']:.3f} ms (min {min(ms_s):.3f} max {max(ms_s):.3f}); "
          f"localise_global median {out['localise_global_ms']['median']:.3f} ms (min {min(ms_l):.3f} max {max(ms_l):.3f}); "
          f"grid {g['W']} x {g['H']} x {A} yaws = {out['leaves']} leaves, {r.n_slice} of {r.n_points} points in the slice", flush=True)
    # the parent's only comparable means: the NDT score of every leaf pose, 65536 poses per call
    if a.cpu_frames:
        cs = np.stack([np.cos(2 * np.pi * np.arange(A) / A), np.sin(2 * np.pi * np.arange(A) / A)], axis=1)
        P = np.tile(np.eye(4), (out["leaves"], 1, 1)).reshape(A, g["H"], g["W"], 4, 4)
        P[..., 0, 0] = P[..., 1, 1] = cs[:, 0, None, None]
        P[..., 1, 0] = cs[:, 1, None, None]
        P[..., 0, 1] = -cs[:, 1, None, None]
        P[..., 0, 3] = g["resolution"] * (g["i0"] + np.arange(g["W"]))[None, None, :]
        P[..., 1, 3] = g["resolution"] * (g["j0"] + np.arange(g["H"]))[None, :, None]
        P = np.ascontiguousarray(P.reshape(-1, 4, 4))
        chunks = [P[c:c + 65536] for c in range(0, len(P), 65536)]
        loc.score_poses(dscans[0], len(dscans[0]), chunks[-1]).result()       # warm-up of the shape
        ms_b, same = [], 0
        for k in range(a.cpu_frames):
            s = dscans[(a.warmup + k) % len(dscans)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parts = [loc.score_poses(s, len(s), c) for c in chunks]
            sc = np.concatenate([p.result()[0] for p in parts])
            ms_b.append((time.perf_counter() - t0) * 1e3)
            r = loc.global_search(s, len(s), A, **kw).result()
            same += int(np.argmax(sc)) == int(r.index[0])
        out["score_poses_all_leaves_ms"] = {"median": med(ms_b), "calls": len(chunks), "frames": a.cpu_frames,
                                            "best_is_the_searchs_best": same}
        print(f"score_poses over all {len(P)} leaf poses in {len(chunks)} calls: median {med(ms_b):.1f} ms per scan (host clock, "
              f"uploads included); its best leaf is the search's on {same} of {a.cpu_frames} frames", flush=True)
    print(json.dumps(out))


def ndt_main(a, scans, dscans, mp, T_init):
    map64 = mp[:, :3].astype(np.float64)
    ScanToMapLocaliser(map64[:1000])                                  # first context of the process: not part of a build time
    icp, icp_build = build_ms(lambda: ScanToMapLocaliser(map64))
    ndt, ndt_build = build_ms(lambda: NDTLocaliser(map64))
    if a.one_frame:
        for k in range(a.warmup):
            ndt.submit(dscans[k % len(dscans)], len(dscans[k % len(dscans)]), T_init).result()
        torch.cuda.synchronize()
        s = dscans[a.warmup % len(dscans)]
        r = ndt.submit(s, len(s), T_init).result()
        print(json.dumps({"one_frame": True, "localiser": "ndt", "status": r.status, "iterations": r.iterations,
                          "n_points": r.n_points}))
        return
    out = {"n_scan": int(np.mean([len(s) for s in scans])), "n_map": len(mp), "n_cells": ndt.n_cells, "frames": a.frames,
           "warmup": a.warmup, "map_build_ms": {"ndt": round(ndt_build, 3), "icp": round(icp_build, 3)}}
    for name, loc in (("ndt", ndt), ("icp", icp)):
        ms, iters, npts, errs = timed_frames(loc, dscans, T_init, a.warmup, a.frames)
        med, it = float(np.median(ms)), float(np.median(iters))
        out[name] = {"ms": {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4)},
                     "iterations": {"median": it, "min": min(iters), "max": max(iters)},
                     "ms_per_iteration": round(med / max(it, 1), 4), "points_after_thinning": int(np.mean(npts)),
                     "max_error_m": round(max(errs), 5), "median_error_m": round(float(np.median(errs)), 5)}
        print(f"{name}  median {med:.3f} ms (min {min(ms):.3f} max {max(ms):.3f}) per frame, iterations median {it:.0f}, "
              f"{out[name]['ms_per_iteration']:.4f} ms per iteration, error median {out[name]['median_error_m']:.4f} m "
              f"max {out[name]['max_error_m']:.4f} m", flush=True)
    print(f"map build: ndt {ndt_build:.2f} ms ({ndt.n_cells} cells), icp grid {icp_build:.2f} ms (host grouping included in both)")
    cmap = NR.cells(map64, ndt.resolution) if a.cpu_frames else None
    for k in range(a.cpu_frames):
        s = scans[(a.warmup + k) % len(scans)]
        t0 = time.perf_counter()
        _, pts = LR.downsample(s, len(s), ndt.leaf, ndt.capacity)
        r = NR.align(pts, cmap, T_init, ndt.iterations, ndt.neighbours, ndt.min_correspondences, ndt.outlier_ratio, ndt.tol_t,
                     ndt.tol_r)
        out["restatement_s"] = round(time.perf_counter() - t0, 2)
        print(f"NDT restatement frame {k}: {out['restatement_s']:.1f} s, {r['iterations']} iterations, status {r['status']}", flush=True)
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(mp)
    for name, loc in (("ndt", ndt), ("icp", icp)):
        loop = LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=VS, epsilon=EPS), loc, np.eye(4))
        t_loop, flagged = [], 0
        for k in range(a.warmup + a.frames):
            t0 = time.perf_counter()
            step = loop.step(scans[k % len(scans)])
            if k >= a.warmup:
                t_loop.append(time.perf_counter() - t0)
                flagged += step.flagged
        out[name]["loop_sps_cvm_ms"] = round(float(np.median(t_loop)) * 1e3, 4)
        out[name]["loop_flagged_frames"] = int(flagged)
        print(f"LocalisationLoop(sps_cvm, {name}) {out[name]['loop_sps_cvm_ms']:.3f} ms per frame ({flagged} flagged)", flush=True)
    print(json.dumps(out))


def ndt_d2d_main(a, scans, dscans, mp, T_init):
    """--source cells: the distribution-to-distribution localiser and the point one on the same frames, alternating frame
    by frame within one run.  Per frame: hipEvent time around submit(), iterations, valid source cells, the error against
    the true pose.  Then the hipEvent time around the source build alone, and LocalisationLoop(SPSCVMFilter, .) with each
    localiser (host wall clock)."""
    map64 = mp[:, :3].astype(np.float64)
    kw = dict(source="cells", source_resolution=a.source_resolution, source_min_points=a.source_min_points)
    locs = {"points": NDTLocaliser(map64), "cells": NDTLocaliser(map64, **kw)}
    if a.one_frame:
        loc = locs["cells"]
        for k in range(a.warmup):
            loc.submit(dscans[k % len(dscans)], len(dscans[k % len(dscans)]), T_init).result()
        torch.cuda.synchronize()
        s = dscans[a.warmup % len(dscans)]
        r = loc.submit(s, len(s), T_init).result()
        print(json.dumps({"one_frame": True, "localiser": "ndt", "source": "cells", "status": r.status,
                          "iterations": r.iterations, "n_points": r.n_points, "n_sources": r.n_sources, "n_corr": r.n_corr}))
        return
    st = torch.cuda.current_stream()
    rec = {name: [] for name in locs}
    for k in range(a.warmup + a.frames):
        s = dscans[k % len(dscans)]
        for name, loc in locs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            pend = loc.submit(s, len(s), T_init)
            e1.record(st)
            r = pend.result()
            e1.synchronize()
            if k >= a.warmup:
                rec[name].append((e0.elapsed_time(e1), r.iterations, r.n_points, r.n_sources, r.n_corr, r.status,
                                  LR.pose_difference(r.pose, np.eye(4))[0]))
    out = {"n_scan": int(np.mean([len(s) for s in scans])), "n_map": len(mp), "n_cells": locs["points"].n_cells,
           "frames": a.frames, "warmup": a.warmup, "source_resolution": locs["cells"].source_resolution,
           "source_min_points": locs["cells"].source_min_points}
    for name, rows in rec.items():
        ms, iters, npts, nsrc, ncorr, status, errs = (list(c) for c in zip(*rows))
        med, it = float(np.median(ms)), float(np.median(iters))
        out[name] = {"ms": {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4)},
                     "iterations": {"median": it, "min": min(iters), "max": max(iters)},
                     "ms_per_iteration": round(med / max(it, 1), 4), "points_after_thinning": int(np.mean(npts)),
                     "n_sources": int(np.median(nsrc)), "n_corr": int(np.median(ncorr)),
                     "status_not_converged": int(sum(v != 0 for v in status)),
                     "max_error_m": round(max(errs), 5), "median_error_m": round(float(np.median(errs)), 5)}
        print(f"{name}  median {med:.3f} ms (min {min(ms):.3f} max {max(ms):.3f}) per frame, iterations median {it:.0f}, "
              f"{out[name]['ms_per_iteration']:.4f} ms per iteration, {out[name]['n_sources']} sources, error median "
              f"{out[name]['median_error_m']:.4f} m max {out[name]['max_error_m']:.4f} m", flush=True)
    # the source build alone: the four memsets and seven launches of one scan's cells, on the thinned points of frame 0
    loc, s = locs["cells"], dscans[0]
    n_pts = torch.zeros(2, dtype=torch.int32, device=loc.device)
    loc._thin(s[:, :3].to(torch.float32).contiguous(), torch.full((1,), len(s), dtype=torch.int32, device=loc.device), len(s),
              n_pts.data_ptr(), st.cuda_stream)
    t_src = []
    for k in range(a.warmup + a.frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        loc._build_sources(n_pts.data_ptr(), st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        if k >= a.warmup:
            t_src.append(e0.elapsed_time(e1))
    out["source_build_ms"] = {"median": round(float(np.median(t_src)), 4), "min": round(min(t_src), 4), "max": round(max(t_src), 4)}
    print(f"source build alone: median {out['source_build_ms']['median']:.4f} ms (min {min(t_src):.4f} max {max(t_src):.4f})", flush=True)
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(mp)
    for name, loc in locs.items():
        loop = LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=VS, epsilon=EPS), loc, np.eye(4))
        t_loop, flagged = [], 0
        for k in range(a.warmup + a.frames):
            t0 = time.perf_counter()
            step = loop.step(scans[k % len(scans)])
            if k >= a.warmup:
                t_loop.append(time.perf_counter() - t0)
                flagged += step.flagged
        out[name]["loop_sps_cvm_ms"] = round(float(np.median(t_loop)) * 1e3, 4)
        out[name]["loop_flagged_frames"] = int(flagged)
        print(f"LocalisationLoop(sps_cvm, ndt {name}) {out[name]['loop_sps_cvm_ms']:.3f} ms per frame ({flagged} flagged)", flush=True)
    print(json.dumps(out))


def ndt_d2d_pyramid_main(a, scans, dscans, mp, T_init):
    """--source cells --resolutions --source-resolutions: the coarse-to-fine registration of the scan's cells
    beside the single cells localiser and the point pyramid on the same frames, alternating frame by frame within one run.
    Per frame: hipEvent time around submit(), slots, live slots per level, valid source cells, the error against the true
    pose.  Then the source build of all levels in one call against one single build per level, alternating too."""
    map64 = mp[:, :3].astype(np.float64)
    res, sres = tuple(float(v) for v in a.resolutions.split(",")), a.source_resolutions
    caps = tuple(int(v) for v in a.level_iterations.split(",")) if a.level_iterations else None
    pkw = dict(resolutions=res, iterations=a.iterations, level_iterations=caps)
    skw = dict(source="cells", source_min_points=a.source_min_points)
    locs = {"cells_pyramid": NDTLocaliser(map64, source_resolutions=sres, **skw, **pkw),
            "cells": NDTLocaliser(map64, source="cells", source_min_points=a.source_min_points
                                  if not isinstance(a.source_min_points, tuple) else None),
            "points_pyramid": NDTLocaliser(map64, **pkw)}
    T0 = LR.perturbation(-a.start_behind, 0.0, 0.0, 0.0) @ T_init
    if a.one_frame:
        loc = locs["cells_pyramid"]
        for k in range(a.warmup):
            loc.submit(dscans[k % len(dscans)], len(dscans[k % len(dscans)]), T0).result()
        torch.cuda.synchronize()
        s = dscans[a.warmup % len(dscans)]
        r = loc.submit(s, len(s), T0).result()
        print(json.dumps({"one_frame": True, "localiser": "ndt", "source": "cells", "resolutions": res, "status": r.status,
                          "iterations": r.iterations, "n_points": r.n_points, "n_sources": r.n_sources, "n_corr": r.n_corr}))
        return
    st = torch.cuda.current_stream()
    L = len(res)
    rec = {name: [] for name in locs}
    for k in range(a.warmup + a.frames):
        s = dscans[k % len(dscans)]
        for name, loc in locs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            pend = loc.submit(s, len(s), T0)
            e1.record(st)
            r = pend.result()
            e1.synchronize()
            if k >= a.warmup:
                per = [int((r.levels == l).sum()) for l in range(L)] if r.levels is not None else [r.iterations]
                rec[name].append((e0.elapsed_time(e1), r.iterations, r.n_points, r.n_sources, r.n_corr, r.status,
                                  LR.pose_difference(r.pose, np.eye(4))[0], per))
    budget = locs["cells_pyramid"].iterations
    out = {"n_scan": int(np.mean([len(s) for s in scans])), "n_map": len(mp), "frames": a.frames, "warmup": a.warmup,
           "resolutions": res, "source_resolutions": sres, "source_min_points": locs["cells_pyramid"].source_level_min_points,
           "budget": budget, "level_iterations": caps, "start_behind_m": a.start_behind}
    for name, rows in rec.items():
        ms, iters, npts, nsrc, ncorr, status, errs, per = (list(c) for c in zip(*rows))
        med, it = float(np.median(ms)), float(np.median(iters))
        out[name] = {"ms": {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4)},
                     "slots": {"median": it, "min": min(iters), "max": max(iters)},
                     "live_slots_per_level": [float(v) for v in np.median(np.array(per), axis=0)],
                     "idle_slots": float(np.median([(budget if name != "cells" else locs[name].iterations) - i for i in iters])),
                     "points_after_thinning": int(np.mean(npts)), "n_sources": int(np.median(nsrc)),
                     "n_corr": int(np.median(ncorr)), "status_not_converged": int(sum(v != 0 for v in status)),
                     "max_error_m": round(max(errs), 5), "median_error_m": round(float(np.median(errs)), 5)}
        print(f"{name}  median {med:.3f} ms (min {min(ms):.3f} max {max(ms):.3f}) per frame, slots median {it:.0f} "
              f"(per level {out[name]['live_slots_per_level']}), {out[name]['n_sources']} sources, error median "
              f"{out[name]['median_error_m']:.4f} m max {out[name]['max_error_m']:.4f} m", flush=True)
    # the source build alone: all levels in one call against one single build per level
    pyr = locs["cells_pyramid"]
    singles = [NDTLocaliser(map64, source="cells", source_resolution=r, source_min_points=m)
               for r, m in zip(pyr.source_resolutions, pyr.source_level_min_points)]
    s = dscans[0]
    n_pts = torch.zeros(2, dtype=torch.int32, device=pyr.device)
    pyr._thin(s[:, :3].to(torch.float32).contiguous(), torch.full((1,), len(s), dtype=torch.int32, device=pyr.device), len(s),
              n_pts.data_ptr(), st.cuda_stream)
    for one in singles:
        one._pts.copy_(pyr._pts)
    t = {"one_call": [], "single_builds": []}
    for k in range(a.warmup + a.frames):
        for name in t:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            if name == "one_call":
                pyr._build_level_sources(n_pts.data_ptr(), st.cuda_stream)
            else:
                for one in singles:
                    one._build_sources(n_pts.data_ptr(), st.cuda_stream)
            e1.record(st)
            e1.synchronize()
            if k >= a.warmup:
                t[name].append(e0.elapsed_time(e1))
    out["source_build_ms"] = {name: round(float(np.median(v)), 4) for name, v in t.items()}
    print(f"source build: {L} levels in one call {out['source_build_ms']['one_call']:.4f} ms, {L} single builds "
          f"{out['source_build_ms']['single_builds']:.4f} ms", flush=True)
    print(json.dumps(out))


def ndt_d2d_pyramid_batch_main(a, scans, dscans, mp, T_init):
    """--d2d-pyramid: see the module docstring.  The sensor stands still at I, so the estimator runs with zero velocity and a
    0.1 s scan period, as in --estimator.  The windows include the host staging of the poses, as in ndt_search_main."""
    from sps_amd.pose_estimator import PoseEstimator
    map64 = mp[:, :3].astype(np.float64)
    res, sres = tuple(float(v) for v in a.resolutions.split(",")), a.source_resolutions
    caps = tuple(int(v) for v in a.level_iterations.split(",")) if a.level_iterations else None
    pkw = dict(resolutions=res, iterations=a.iterations, level_iterations=caps)
    cells = NDTLocaliser(map64, source="cells", source_resolutions=sres, source_min_points=a.source_min_points, **pkw)
    points = NDTLocaliser(map64, **pkw)
    st = torch.cuda.current_stream()
    I4 = np.eye(4)
    stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out = {"frames": a.frames, "warmup": a.warmup, "n_map": len(mp), "resolutions": res, "source_resolutions": sres,
           "source_min_points": cells.source_level_min_points, "budget": a.iterations, "level_iterations": caps}

    def alternate(calls):
        """hipEvent time around every call of ``calls`` (name -> function of the frame's scan that returns the last pending
        object it issued), the order swapped every frame -> name -> (ms per frame, the last result)"""
        t, last = {n: [] for n in calls}, {}
        for k in range(a.warmup + a.frames):
            s = dscans[k % len(dscans)]
            for n in (tuple(calls) if k % 2 == 0 else tuple(calls)[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                pend = calls[n](s)
                e1.record(st)
                last[n] = pend.result()
                e1.synchronize()
                if k >= a.warmup:
                    t[n].append(e0.elapsed_time(e1))
        return t, last

    for K in (8, 64):
        starts = hypothesis_starts(T_init, K)

        def sequential(s):
            for T in starts:
                pend = cells.submit(s, len(s), T)
            return pend
        t, last = alternate({"d2d_pyramid_batch": lambda s: cells.submit_batch(s, len(s), starts, d2d_pyramid=True),
                             "sequential_submits": sequential,
                             "point_pyramid_batch": lambda s: points.submit_batch(s, len(s), starts, coarse_to_fine=True)})
        rows = {n: stats(v) for n, v in t.items()}
        for n in ("d2d_pyramid_batch", "point_pyramid_batch"):
            r = last[n]
            rows[n].update(best=r.best, slots_max=max(p.iterations for p in r.results),
                           error_m=round(LR.pose_difference(r.pose, I4)[0], 5))
        rows["d2d_pyramid_batch"].update(score_level=last["d2d_pyramid_batch"].score_level,
                                         n_sources=last["d2d_pyramid_batch"].n_sources)
        out[f"k{K}"] = rows
        print(f"K = {K}: submit_batch(d2d_pyramid) median {rows['d2d_pyramid_batch']['median']:.3f} ms (scores on level "
              f"{rows['d2d_pyramid_batch']['score_level']}, {rows['d2d_pyramid_batch']['n_sources']} sources, error "
              f"{rows['d2d_pyramid_batch']['error_m']:.4f} m); {K} submits median {rows['sequential_submits']['median']:.3f} ms; "
              f"point pyramid's batch median {rows['point_pyramid_batch']['median']:.3f} ms (error "
              f"{rows['point_pyramid_batch']['error_m']:.4f} m)", flush=True)
    if a.search:
        poses = search_poses(T_init, a.search)
        t, last = alternate({"d2d_pyramid": lambda s: cells.relocalise(s, len(s), poses, keep=8, d2d_pyramid=True),
                             "point_pyramid": lambda s: points.relocalise(s, len(s), poses, keep=8, coarse_to_fine=True)})
        out[f"relocalise_P{a.search}_keep8"] = {n: dict(stats(v), index=last[n].index,
                                                        error_m=round(LR.pose_difference(last[n].pose, I4)[0], 5))
                                                for n, v in t.items()}
        print(f"relocalise over {a.search} poses, keep 8: d2d_pyramid median {np.median(t['d2d_pyramid']):.3f} ms, point pyramid "
              f"median {np.median(t['point_pyramid']):.3f} ms", flush=True)
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(mp)

    def make_loop(device_guess):
        return LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=VS, epsilon=EPS), cells, I4, estimator=PoseEstimator(I4, "cuda"),
                                device_guess=device_guess, d2d_pyramid=True)
    loops = {"d2d_pyramid_device": make_loop(True), "d2d_pyramid_host": make_loop(False)}
    t_loop, flagged = {m: [] for m in loops}, {m: 0 for m in loops}
    for k in range(a.warmup + a.frames):
        for m in (tuple(loops) if k % 2 == 0 else tuple(loops)[::-1]):
            t0 = time.perf_counter()
            step = loops[m].step(scans[k % len(scans)], dt=0.1)
            if k >= a.warmup:
                t_loop[m].append((time.perf_counter() - t0) * 1e3)
                flagged[m] += step.flagged
    for m in loops:
        out[f"loop_{m}_ms"] = stats(t_loop[m])
        out[f"loop_{m}_flagged"] = int(flagged[m])
        print(f"LocalisationLoop(sps_cvm, cells pyramid, ukf, d2d_pyramid) {m:18s} median {out[f'loop_{m}_ms']['median']:.3f} ms "
              f"per frame (min {min(t_loop[m]):.3f} max {max(t_loop[m]):.3f}; {flagged[m]} flagged)", flush=True)
    print(json.dumps(out))


def ndt_d2d_batch_main(a, scans, dscans, mp, T_init):
    """--source cells --d2d: the calls that take several poses, distribution to distribution against the point path, the two
    alternating frame by frame in one run, hipEvents around each call (the windows include the host staging of the poses, as
    in ndt_search_main).  --search P: score_poses and relocalise(keep=8); --hypotheses K: submit_batch; --estimator: the loop
    with the UKF per frame (host wall clock), cells on the device path (d2d), cells on the host path, points on the device
    path."""
    from sps_amd.pose_estimator import PoseEstimator
    map64 = mp[:, :3].astype(np.float64)
    kw = dict(source="cells", source_resolution=a.source_resolution, source_min_points=a.source_min_points)
    locs = {"points": (NDTLocaliser(map64), {}), "cells": (NDTLocaliser(map64, **kw), dict(d2d=True))}
    st = torch.cuda.current_stream()
    stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out = {"frames": a.frames, "warmup": a.warmup, "n_cells": locs["points"][0].n_cells}

    def timed(call):
        """-> (ms, result) of one call, hipEvents around its issue"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        pend = call()
        e1.record(st)
        r = pend.result()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def alternate(what, make):
        """make(loc, extra, scan) -> a pending call; both localisers per frame, the order swapped every frame"""
        ms, last = {n: [] for n in locs}, {}
        for k in range(a.warmup + a.frames):
            s = dscans[k % len(dscans)]
            for n in (tuple(locs) if k % 2 == 0 else tuple(locs)[::-1]):
                t, last[n] = timed(lambda: make(*locs[n], s))
                if k >= a.warmup:
                    ms[n].append(t)
        out[what] = {n: stats(v) for n, v in ms.items()}
        out[what]["ratio_points_over_cells"] = round(out[what]["points"]["median"] / out[what]["cells"]["median"], 3)
        print(f"{what}: points median {out[what]['points']['median']:.3f} ms (min {min(ms['points']):.3f} max {max(ms['points']):.3f}), "
              f"cells d2d median {out[what]['cells']['median']:.3f} ms (min {min(ms['cells']):.3f} max {max(ms['cells']):.3f}), "
              f"ratio {out[what]['ratio_points_over_cells']:.2f}", flush=True)
        return last

    if a.search:
        poses = search_poses(T_init, a.search)
        if a.one_frame:
            for n, (loc, extra) in locs.items():
                for k in range(max(a.warmup, 1)):
                    loc.submit(dscans[k % len(dscans)], len(dscans[k % len(dscans)]), T_init).result()
                torch.cuda.synchronize()
                sc, cnt = loc.score_poses(dscans[0], len(dscans[0]), poses, **extra).result()
                print(json.dumps({"one_frame": True, "path": n, "search": a.search, "best": int(np.argmax(sc)), "count_max": int(cnt.max())}))
            return
        last = alternate(f"score_poses_P{a.search}", lambda loc, extra, s: loc.score_poses(s, len(s), poses, **extra))
        out["score_best_index"] = {n: int(np.argmax(r[0])) for n, r in last.items()}
        out["score_count_max"] = {n: int(r[1].max()) for n, r in last.items()}
        last = alternate(f"relocalise_P{a.search}_keep8", lambda loc, extra, s: loc.relocalise(s, len(s), poses, keep=8, **extra))
        out["relocalise"] = {n: {"index": r.index, "status": r.batch.results[max(r.batch.best, 0)].status,
                                 "error_m": round(LR.pose_difference(r.pose, np.eye(4))[0], 5)} for n, r in last.items()}
    if a.hypotheses:
        starts = hypothesis_starts(T_init, a.hypotheses)
        last = alternate(f"submit_batch_K{a.hypotheses}", lambda loc, extra, s: loc.submit_batch(s, len(s), starts, **extra))
        out["batch"] = {n: {"best": r.best, "iterations_max": max(x.iterations for x in r.results),
                            "iterations_sum": sum(x.iterations for x in r.results), "n_points": r.results[0].n_points,
                            "n_sources": r.results[0].n_sources,
                            "error_m": round(LR.pose_difference(r.pose, np.eye(4))[0], 5)} for n, r in last.items()}
    if a.estimator:
        net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
        mpt = torch.from_numpy(mp)
        I4 = np.eye(4)

        def make_loop(n, **lkw):
            return LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=VS, epsilon=EPS), locs[n][0], I4,
                                    estimator=PoseEstimator(I4, "cuda"), **lkw)
        loops = {"cells_d2d_device": make_loop("cells", d2d=True), "cells_host": make_loop("cells"),
                 "points_device": make_loop("points")}
        assert [l.device_guess for l in loops.values()] == [True, False, True]
        t_loop, flagged = {m: [] for m in loops}, {m: 0 for m in loops}
        for k in range(a.warmup + a.frames):
            order = tuple(loops) if k % 2 == 0 else tuple(loops)[::-1]
            for m in order:                                          # alternating: all see the same machine state
                t0 = time.perf_counter()
                step = loops[m].step(scans[k % len(scans)], dt=0.1)
                if k >= a.warmup:
                    t_loop[m].append((time.perf_counter() - t0) * 1e3)
                    flagged[m] += step.flagged
        for m in loops:
            out[f"loop_{m}_ms"] = stats(t_loop[m])
            out[f"loop_{m}_flagged"] = int(flagged[m])
            print(f"LocalisationLoop(sps_cvm, ndt, ukf) {m:17s} median {out[f'loop_{m}_ms']['median']:.3f} ms per frame (min "
                  f"{min(t_loop[m]):.3f} max {max(t_loop[m]):.3f}; {flagged[m]} flagged)", flush=True)
    print(json.dumps(out))


def ndt_pyramid_main(a, dscans, mp, T_init):
    """--resolutions: the pyramid localiser and the single-map one on the same frames, alternating in blocks within one
    session, from the tool's usual start and from a start 0.5 m behind along the corridor (the case the pyramid is for).
    Per frame: hipEvent time around submit(), the live slots (those that did work) and the idle ones (budget - live, whose
    launches return at once), the slots per level, the error against the true pose.  Then the build times: every level's
    map alone (a single-map localiser at that resolution) and the pyramid localiser (its single map + the levels)."""
    res = tuple(float(v) for v in a.resolutions.split(","))
    caps = tuple(int(v) for v in a.level_iterations.split(",")) if a.level_iterations else None
    map64 = mp[:, :3].astype(np.float64)
    ScanToMapLocaliser(map64[:1000])                                  # first context of the process: not part of a build time
    single, single_build = build_ms(lambda: NDTLocaliser(map64))
    pyr, pyr_build = build_ms(lambda: NDTLocaliser(map64, resolutions=res, iterations=a.iterations, level_iterations=caps))
    level_build = []
    for r in res:
        one, ms = build_ms(lambda: NDTLocaliser(map64, resolution=r))
        level_build.append({"resolution": r, "cells": one.n_cells, "ms": round(ms, 3)})
        del one
    out = {"n_map": len(mp), "frames": a.frames, "warmup": a.warmup, "resolutions": res, "budget": a.iterations,
           "level_iterations": caps, "level_cells": pyr.level_cells,
           "build_ms": {"single": round(single_build, 3), "pyramid_localiser": round(pyr_build, 3), "levels": level_build}}
    st = torch.cuda.current_stream()
    for start_name, T0 in (("usual", T_init), ("lag_0.5m", LR.perturbation(0.5, 0.0, 0.0, 0.0))):
        rec = {"single": [], "pyramid": []}
        for k in range(a.warmup + a.frames):
            s = dscans[k % len(dscans)]
            for name, loc in (("single", single), ("pyramid", pyr)):   # alternating: both see the same machine state
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                pend = loc.submit(s, len(s), T0)
                e1.record(st)
                r = pend.result()
                e1.synchronize()
                if k >= a.warmup:
                    lv = np.bincount(r.levels, minlength=len(res)) if r.levels is not None else None
                    rec[name].append((e0.elapsed_time(e1), r.iterations, r.status, LR.pose_difference(r.pose, np.eye(4))[0], lv))
        out[start_name] = {}
        for name, rows in rec.items():
            ms, live = [v[0] for v in rows], [v[1] for v in rows]
            budget = a.iterations if name == "pyramid" else single.iterations
            d = {"ms": {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)},
                 "live_slots": {"median": float(np.median(live)), "min": min(live), "max": max(live)},
                 "idle_slots_median": float(budget - np.median(live)),
                 "status_counts": {str(c): int(sum(v[2] == c for v in rows)) for c in sorted({v[2] for v in rows})},
                 "error_m": {"median": round(float(np.median([v[3] for v in rows])), 5), "max": round(max(v[3] for v in rows), 5)}}
            if name == "pyramid":
                d["slots_per_level_median"] = [float(x) for x in np.median(np.stack([v[4] for v in rows]), axis=0)]
            out[start_name][name] = d
            print(f"{start_name:9s} {name:8s} median {d['ms']['median']:.3f} ms (min {d['ms']['min']:.3f} max {d['ms']['max']:.3f}) per "
                  f"frame, live slots median {d['live_slots']['median']:.0f} of {budget} (idle {d['idle_slots_median']:.0f}), status "
                  f"{d['status_counts']}, error median {d['error_m']['median']:.4f} m max {d['error_m']['max']:.4f} m"
                  + (f", slots per level {d['slots_per_level_median']}" if name == "pyramid" else ""), flush=True)
    print("map builds (host grouping included): single localiser " + f"{single_build:.2f} ms, pyramid localiser {pyr_build:.2f} ms; "
          + ", ".join(f"{b['resolution']} m: {b['ms']:.2f} ms ({b['cells']} cells)" for b in level_build))
    print(json.dumps(out))


def hypothesis_starts(T_init, K):
    """K start poses around T_init: the guess itself, then offsets 0.5 m apart along and across, outwards, in the order
    pose_grid gives a 9 x 9 grid sorted by distance (so a smaller K is a prefix of a larger one)."""
    from sps_amd.localiser import pose_grid
    g = pose_grid([0.5 * i for i in range(-4, 5)], [0.5 * i for i in range(-4, 5)], 0.0)
    order = np.argsort(np.hypot(g[:, 0, 3], g[:, 1, 3]), kind="stable")
    return np.stack([T_init @ g[k] for k in order[:K]])


def ndt_batch_main(a, dscans, mp, T_init):
    """--hypotheses K: hipEvent time around one submit_batch of K start poses against K back-to-back submit calls from the
    same poses, interleaved frame by frame in one run."""
    K = a.hypotheses
    ndt = NDTLocaliser(mp[:, :3].astype(np.float64))
    starts = hypothesis_starts(T_init, K)
    st = torch.cuda.current_stream()
    if a.one_frame:
        for k in range(a.warmup):
            ndt.submit_batch(dscans[k % len(dscans)], len(dscans[k % len(dscans)]), starts).result()
        torch.cuda.synchronize()
        s = dscans[a.warmup % len(dscans)]
        r = ndt.submit_batch(s, len(s), starts).result()
        print(json.dumps({"one_frame": True, "localiser": "ndt", "hypotheses": K, "best": r.best,
                          "iterations": [p.iterations for p in r.results], "n_points": r.results[0].n_points}))
        return
    t_batch, t_single, t_one, iters, best, errs = [], [], [], [], [], []
    for k in range(a.warmup + a.frames):
        s = dscans[k % len(dscans)]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(st)
        pend = ndt.submit_batch(s, len(s), starts)
        e[1].record(st)
        r = pend.result()
        e[2].record(st)
        singles = [ndt.submit(s, len(s), T) for T in starts]
        e[3].record(st)
        singles = [p.result() for p in singles]
        e[3].synchronize()
        assert all(x.pose.tobytes() == y.pose.tobytes() and x.iterations == y.iterations for x, y in zip(r.results, singles))
        if k >= a.warmup:
            t_batch.append(e[0].elapsed_time(e[1]))
            t_single.append(e[2].elapsed_time(e[3]))
            iters.append(max(p.iterations for p in r.results))
            best.append(r.best)
            errs.append(LR.pose_difference(r.pose, np.eye(4))[0])
    for k in range(a.warmup + a.frames):                                   # one submit from the guess: the K = 1 yardstick
        s = dscans[k % len(dscans)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        pend = ndt.submit(s, len(s), starts[0])
        e1.record(st)
        pend.result()
        e1.synchronize()
        if k >= a.warmup:
            t_one.append(e0.elapsed_time(e1))
    mb, ms, m1, it = float(np.median(t_batch)), float(np.median(t_single)), float(np.median(t_one)), float(np.median(iters))
    out = {"hypotheses": K, "frames": a.frames, "warmup": a.warmup,
           "batch_ms": {"median": round(mb, 4), "min": round(min(t_batch), 4), "max": round(max(t_batch), 4)},
           "k_single_ms": {"median": round(ms, 4), "min": round(min(t_single), 4), "max": round(max(t_single), 4)},
           "one_submit_ms": {"median": round(m1, 4), "min": round(min(t_one), 4), "max": round(max(t_one), 4)},
           "iterations_max_over_hypotheses_median": it, "batch_ms_per_iteration": round(mb / max(it, 1), 4),
           "speedup": round(ms / mb, 3), "best": sorted(set(best)), "max_error_m": round(max(errs), 5)}
    print(f"K = {K}: submit_batch median {mb:.3f} ms (min {min(t_batch):.3f} max {max(t_batch):.3f}), {K} x submit median "
          f"{ms:.3f} ms, one submit {m1:.3f} ms; {it:.0f} iterations (longest hypothesis), {out['batch_ms_per_iteration']:.4f} ms "
          f"per iteration; best {out['best']}, error of the selected pose max {out['max_error_m']:.4f} m", flush=True)
    print(json.dumps(out))


def search_poses(T_init, P):
    """P poses T_init @ D(a, b, psi) of a planar grid of +-3 m along, +-1 m across and +-15 degrees"""
    from sps_amd.localiser import pose_grid
    side = max(int(np.ceil((P / 3.0) ** 0.5)), 1)
    g = pose_grid(np.linspace(-3.0, 3.0, side), np.linspace(-1.0, 1.0, 3), np.linspace(-15.0, 15.0, side))
    return np.stack([T_init @ d for d in g[:P]])


def ndt_search_main(a, dscans, mp, T_init):
    """--search P: hipEvent time around one score_poses of P poses against ceil(P / 64) submit_batch(iterations=0) calls
    over the same poses (each thins the scan again: there is no other way to reach the batch's final scores), interleaved
    frame by frame in one run; the two must agree bit for bit.  Both windows include their host staging (the pinned copy of
    the poses and the zeroed output buffer: once for P poses on one side, once per 64 poses on the other), so the ratio is
    that of the calls as a user makes them, not of the kernels alone; a kernel trace gives those."""
    P = a.search
    ndt = NDTLocaliser(mp[:, :3].astype(np.float64))
    poses = search_poses(T_init, P)
    st = torch.cuda.current_stream()
    t_score, t_batch, npts = [], [], 0
    for k in range(a.warmup + a.frames):
        s = dscans[k % len(dscans)]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(st)
        pend = ndt.score_poses(s, len(s), poses)
        e[1].record(st)
        scores, counts = pend.result()
        e[2].record(st)
        batches = [ndt.submit_batch(s, len(s), poses[lo:lo + 64], iterations=0) for lo in range(0, P, 64)]
        e[3].record(st)
        batches = [b.result() for b in batches]
        e[3].synchronize()
        assert np.concatenate([b.scores for b in batches]).tobytes() == scores.tobytes()
        assert np.concatenate([b.counts for b in batches]).tobytes() == counts.tobytes()
        npts = batches[0].results[0].n_points
        if k >= a.warmup:
            t_score.append(e[0].elapsed_time(e[1]))
            t_batch.append(e[2].elapsed_time(e[3]))
    ms, mb = float(np.median(t_score)), float(np.median(t_batch))
    out = {"search": P, "frames": a.frames, "warmup": a.warmup, "n_points": npts,
           "score_poses_ms": {"median": round(ms, 4), "min": round(min(t_score), 4), "max": round(max(t_score), 4)},
           "batch0_ms": {"median": round(mb, 4), "min": round(min(t_batch), 4), "max": round(max(t_batch), 4)},
           "batch0_calls": (P + 63) // 64, "ratio_batch0_over_score": round(mb / ms, 3), "bits_agree": True}
    print(f"P = {P}: score_poses median {ms:.3f} ms (min {min(t_score):.3f} max {max(t_score):.3f}), {(P + 63) // 64} x "
          f"submit_batch(iterations=0) median {mb:.3f} ms (min {min(t_batch):.3f} max {max(t_batch):.3f}); {npts} points; the "
          f"bits agree", flush=True)
    print(json.dumps(out))


def ndt_update_main(a, dscans, mp, T_init):
    """--update-map: per frame, in one run and in this order: submit (hipEvents), sps_ndt_map_update alone on the points that
    submit left thinned, at the true pose (hipEvents), submit(integrate=True) (hipEvents), and a new NDTLocaliser over the
    map and the frame's thinned points (host wall clock between two device synchronisations: the constructor groups on the
    host and synchronises; the union is prepared outside the window).  The online map keeps growing over the run: the same
    12 scans come back, so after the first round every update merges into existing cells."""
    map64 = mp[:, :3].astype(np.float64)
    static = NDTLocaliser(map64)
    cap_cells = 2 * static.n_cells
    ndt, build = build_ms(lambda: NDTLocaliser(map64, cell_capacity=cap_cells))
    st = torch.cuda.current_stream()
    I4 = np.eye(4)
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    n_pts = torch.zeros(1, dtype=torch.int32, device="cuda")
    if a.one_frame:
        for k in range(a.warmup):
            ndt.submit(dscans[k % len(dscans)], len(dscans[k % len(dscans)]), T_init, integrate=True).result()
        torch.cuda.synchronize()
        s = dscans[a.warmup % len(dscans)]
        r = ndt.submit(s, len(s), T_init, integrate=True).result()
        print(json.dumps({"one_frame": True, "localiser": "ndt", "update_map": True, "status": r.status, "iterations": r.iterations,
                          "n_points": r.n_points, "map_update": vars(r.map_update)}))
        return
    t_submit, t_update, t_both, t_rebuild, last = [], [], [], [], None
    for k in range(a.warmup + a.frames):
        s = dscans[k % len(dscans)]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        e[0].record(st)
        pend = ndt.submit(s, len(s), T_init)
        e[1].record(st)
        r = pend.result()
        n_pts.fill_(r.n_points)
        e[2].record(st)
        ndt._update(n_pts.data_ptr(), I4, None, None, 0, info.data_ptr(), st.cuda_stream)
        e[3].record(st)
        union = np.concatenate([map64, ndt._pts[:r.n_points].cpu().numpy()])   # the sensor sits at I: sensor frame = map frame
        e[4].record(st)
        pend = ndt.submit(s, len(s), T_init, integrate=True)
        e[5].record(st)
        last = pend.result()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rebuilt = NDTLocaliser(union)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        del rebuilt
        if k >= a.warmup:
            t_submit.append(e[0].elapsed_time(e[1]))
            t_update.append(e[2].elapsed_time(e[3]))
            t_both.append(e[4].elapsed_time(e[5]))
            t_rebuild.append((t1 - t0) * 1e3)

    def stats(v):
        return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out = {"frames": a.frames, "warmup": a.warmup, "n_map": len(mp), "cells_at_build": static.n_cells, "cell_capacity": cap_cells,
           "dynamic_build_ms": round(build, 3), "n_points": last.n_points, "map_info": ndt.map_info(),
           "last_update": vars(last.map_update), "submit_ms": stats(t_submit), "update_alone_ms": stats(t_update),
           "submit_integrate_ms": stats(t_both), "rebuild_wall_ms": stats(t_rebuild)}
    out["rebuild_over_update"] = round(out["rebuild_wall_ms"]["median"] / out["update_alone_ms"]["median"], 1)
    for name in ("submit_ms", "update_alone_ms", "submit_integrate_ms", "rebuild_wall_ms"):
        print(f"{name:22s} median {out[name]['median']:.4f} (min {out[name]['min']:.4f} max {out[name]['max']:.4f})", flush=True)
    print(json.dumps(out))


def ndt_carve_main(a, scans, dscans, mp, T_init):
    """--carve: per frame, in one run and in this order (hipEvents around each): submit; sps_ndt_map_carve alone on the points
    that submit left thinned, at the true pose; sps_ndt_map_update alone on the same points; submit(integrate=True,
    carve=True).  The 12 scans come back, so the map and the carve's counters reach a steady state within the warm-up."""
    from sps_amd.localiser import CARVE_DEFAULTS
    map64 = mp[:, :3].astype(np.float64)
    n_cells = NDTLocaliser(map64).n_cells
    ndt = NDTLocaliser(map64, cell_capacity=2 * n_cells)
    opts = ndt._check_carve(True, dict(CARVE_DEFAULTS))
    st = torch.cuda.current_stream()
    I4 = np.eye(4)
    info = torch.zeros(8, dtype=torch.int32, device="cuda")
    n_pts = torch.zeros(1, dtype=torch.int32, device="cuda")
    if a.one_frame:
        for k in range(a.warmup):
            ndt.submit(dscans[k % len(dscans)], len(dscans[k % len(dscans)]), T_init, integrate=True, carve=True).result()
        torch.cuda.synchronize()
        s = dscans[a.warmup % len(dscans)]
        r = ndt.submit(s, len(s), T_init, integrate=True, carve=True).result()
        print(json.dumps({"one_frame": True, "localiser": "ndt", "carve": True, "status": r.status, "iterations": r.iterations,
                          "n_points": r.n_points, "map_carve": vars(r.map_carve), "map_update": vars(r.map_update)}))
        return
    t = {"submit_ms": [], "carve_alone_ms": [], "update_alone_ms": [], "submit_integrate_carve_ms": []}
    cut, cleared, last = 0, 0, None
    for k in range(a.warmup + a.frames):
        s = dscans[k % len(dscans)]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        e[0].record(st)
        pend = ndt.submit(s, len(s), T_init)
        e[1].record(st)
        r = pend.result()
        n_pts.fill_(r.n_points)
        e[2].record(st)
        ndt._carve(n_pts.data_ptr(), I4, None, None, opts, info.data_ptr(), st.cuda_stream)
        e[3].record(st)
        e[4].record(st)
        ndt._update(n_pts.data_ptr(), I4, None, None, 0, info.data_ptr() + 16, st.cuda_stream)
        e[5].record(st)
        alone = info.cpu().numpy()
        e[6].record(st)
        pend = ndt.submit(s, len(s), T_init, integrate=True, carve=True)
        e[7].record(st)
        last = pend.result()
        torch.cuda.synchronize()
        if k >= a.warmup:
            for i, name in enumerate(t):
                t[name].append(e[2 * i].elapsed_time(e[2 * i + 1]))
            cut += int(alone[3]) + last.map_carve.cut
            cleared += int(alone[2]) + last.map_carve.cleared

    def stats(v):
        return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out = {"frames": a.frames, "warmup": a.warmup, "n_map": len(mp), "cells_at_build": n_cells, "n_points": last.n_points,
           "carve_options": opts, "map_info": ndt.map_info(), "last_carve": vars(last.map_carve), "rays_cut_in_all_timed_carves": cut,
           "cells_cleared_in_all_timed_carves": cleared}
    for name, v in t.items():
        out[name] = stats(v)
        print(f"{name:26s} median {out[name]['median']:.4f} (min {out[name]['min']:.4f} max {out[name]['max']:.4f})", flush=True)
    if a.cpu_frames:
        from tests import ndt_carve_reference as CR
        from tests import ndt_update_reference as UR
        sc = scans[a.warmup % len(scans)]
        _, pts = LR.downsample(sc, len(sc), ndt.leaf, ndt.capacity)
        visited = []
        ref = CR.carve(UR.build(map64, 2 * n_cells), pts, I4, visited=visited)
        out["restatement_one_frame"] = {"info": ref, "cells_per_ray_mean": round(float(np.mean(visited)), 2),
                                        "cells_per_ray_max": int(max(visited))}
        print(f"restatement, one frame on the built map: info {ref}, cells per ray mean {np.mean(visited):.2f} max {max(visited)}", flush=True)
    print(json.dumps(out))


def ndt_online_pyramid_main(a, dscans, mp, T_init):
    """--resolutions with --integrate / --carve: the online pyramid's fused calls against the only way without them, one
    single-map online localiser per level doing the same work one after another.  Per frame, in one run and in this order
    (hipEvents around each): the pyramid's submit; sps_ndt_pyramid_update alone on the points that submit left thinned, at
    the true pose; the L sps_ndt_map_update calls on the same points; sps_ndt_pyramid_carve alone; the L sps_ndt_map_carve
    calls; submit(integrate=True, carve=True).  Both sides see the same points at the same poses, so their maps stay equal;
    the 12 scans come back, so the maps and the carve's counters reach a steady state within the warm-up."""
    from sps_amd.localiser import CARVE_DEFAULTS
    map64 = mp[:, :3].astype(np.float64)
    res = tuple(float(v) for v in a.resolutions.split(","))
    caps = tuple(int(v) for v in a.level_iterations.split(",")) if a.level_iterations else None
    cells = [len(np.unique(np.floor(map64 / r).astype(np.int64), axis=0)) for r in res]
    level_caps = tuple(max(2 * c, 4096) for c in cells)
    pyr = NDTLocaliser(map64, resolutions=res, iterations=a.iterations, level_iterations=caps, level_capacities=level_caps)
    singles = [NDTLocaliser(map64, resolution=r, cell_capacity=c) for r, c in zip(res, level_caps)]
    L = len(res)
    opts = pyr._check_carve(True, dict(CARVE_DEFAULTS))
    sopts = [s._check_carve(True, dict(CARVE_DEFAULTS)) for s in singles]
    st = torch.cuda.current_stream()
    I4 = np.eye(4)
    info = torch.zeros(4 * 4 * L, dtype=torch.int32, device="cuda")           # fused update | chained | fused carve | chained
    n_pts = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = {}
    if a.update_map:
        kw["integrate"] = True
    if a.carve:
        kw["carve"] = True
    names = ["submit_ms"] + (["update_fused_ms", "update_chained_ms"] if a.update_map else []) + \
        (["carve_fused_ms", "carve_chained_ms"] if a.carve else []) + ["submit_online_ms"]
    t = {n: [] for n in names}
    last = None
    pts, cap = pyr._pts.data_ptr(), pyr.capacity
    for k in range(a.warmup + a.frames):
        s = dscans[k % len(dscans)]
        ev = {n: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for n in names}
        ev["submit_ms"][0].record(st)
        pend = pyr.submit(s, len(s), T_init)
        ev["submit_ms"][1].record(st)
        n_pts.fill_(pend.result().n_points)
        n_ptr, base = n_pts.data_ptr(), info.data_ptr()
        if a.carve:                                                  # the carve before the update, as submit orders them
            ev["carve_fused_ms"][0].record(st)
            pyr._carve(n_ptr, I4, None, None, opts, base + 2 * 16 * L, st.cuda_stream)
            ev["carve_fused_ms"][1].record(st)
            ev["carve_chained_ms"][0].record(st)
            for l, one in enumerate(singles):
                o = sopts[l]
                one.ctx.ndt_map_carve(pts, n_ptr, cap, I4, None, None, o["end_margin"], o["through_sigma"], o["min_pass"],
                                      o["miss_frames"], o["max_steps"], base + 3 * 16 * L + 16 * l, None, st.cuda_stream)
            ev["carve_chained_ms"][1].record(st)
        if a.update_map:
            ev["update_fused_ms"][0].record(st)
            pyr._update(n_ptr, I4, None, None, 0, base, st.cuda_stream)
            ev["update_fused_ms"][1].record(st)
            ev["update_chained_ms"][0].record(st)
            for l, one in enumerate(singles):
                one.ctx.ndt_map_update(pts, n_ptr, cap, I4, None, None, 0, base + 16 * L + 16 * l, one._update_scratch.data_ptr(),
                                       st.cuda_stream)
            ev["update_chained_ms"][1].record(st)
        words = info.cpu().numpy().reshape(4, L, 4)
        assert (words[0] == words[1]).all() and (words[2] == words[3]).all(), "fused and chained calls disagree"
        ev["submit_online_ms"][0].record(st)
        pend = pyr.submit(s, len(s), T_init, **kw)
        ev["submit_online_ms"][1].record(st)
        last = pend.result()
        if last.status in (0, 1):                                    # untimed: the single maps follow, at the pose the device found
            for l, one in enumerate(singles):
                o = sopts[l]
                if a.carve:
                    one.ctx.ndt_map_carve(pts, n_ptr, cap, last.pose, None, None, o["end_margin"], o["through_sigma"], o["min_pass"],
                                          o["miss_frames"], o["max_steps"], base + 3 * 16 * L + 16 * l, None, st.cuda_stream)
                if a.update_map:
                    one.ctx.ndt_map_update(pts, n_ptr, cap, last.pose, None, None, 0, base + 16 * L + 16 * l,
                                           one._update_scratch.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        if k >= a.warmup:
            for n in names:
                t[n].append(ev[n][0].elapsed_time(ev[n][1]))

    def stats(v):
        return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out = {"frames": a.frames, "warmup": a.warmup, "n_map": len(mp), "resolutions": res, "cells_at_build": cells,
           "level_capacities": level_caps, "n_points": last.n_points, "slots": last.iterations,
           "level_info": [pyr.pyramid_info(l) for l in range(L)],
           "last_update": [vars(u) for u in last.map_update] if last.map_update else None,
           "last_carve": [vars(c) for c in last.map_carve] if last.map_carve else None}
    for name, v in t.items():
        out[name] = stats(v)
        print(f"{name:22s} median {out[name]['median']:.4f} (min {out[name]['min']:.4f} max {out[name]['max']:.4f})", flush=True)
    print(json.dumps(out))


def ndt_estimator_main(a, scans, dscans, mp, T_init):
    """--estimator: the estimator's calls under hipEvents, then the loop with and without it (see the module docstring).
    The sensor stands still at I, so the estimator runs with zero velocity and a 0.1 s scan period."""
    from sps_amd import _native
    from sps_amd.pose_estimator import PoseEstimator
    map64 = mp[:, :3].astype(np.float64)
    ndt = NDTLocaliser(map64)
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(mp)
    st = torch.cuda.current_stream()
    I4 = np.eye(4)

    def make_loop(mode):
        est = None if mode == "none" else PoseEstimator(I4, "cuda")
        return LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=VS, epsilon=EPS), ndt, I4, estimator=est,
                                device_guess=None if mode == "none" else mode == "device")

    if a.one_frame:
        loop = make_loop("device")
        for k in range(a.warmup):
            loop.step(scans[k % len(scans)], dt=0.1)
        torch.cuda.synchronize()
        step = loop.step(scans[a.warmup % len(scans)], imu=synthetic.sequence_imu(2, step=0.0, rate=100.0)[1])
        print(json.dumps({"one_frame": True, "localiser": "ndt", "estimator": True, "status": step.pose_result.status,
                          "iterations": step.pose_result.iterations, "flagged": bool(step.flagged)}))
        return

    def stats(v):
        return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out = {"frames": a.frames, "warmup": a.warmup, "n_map": len(mp)}
    est = PoseEstimator(I4, "cuda")
    T_meas = torch.from_numpy(np.ascontiguousarray(LR.perturbation(0.01, -0.01, 0.0, 0.1))).cuda()
    rows = {M: synthetic.sequence_imu(2, step=0.0, scan_period=0.1, rate=10.0 * M)[1] for M in (1, 10, 40)}
    drows = {M: torch.from_numpy(r).cuda() for M, r in rows.items()}
    t = {}

    def kernel_only(M):
        _native.check(_native.lib.sps_ukf_predict(est._state_ptr, drows[M].data_ptr(), M, est._Q, est._pred_ptr, est._pinfo_ptr,
                                                  st.cuda_stream))
    calls = [(f"predict_kernel_M{M}", lambda M=M: kernel_only(M)) for M in (1, 10, 40)]
    calls += [(f"predict_imu_M{M}", lambda M=M: est.predict_imu(rows[M])) for M in (1, 10, 40)]
    calls += [("predict_dt", lambda: est.predict(0.1))]
    for k in range(a.warmup + a.frames):
        for name, call in calls:                                     # a correction behind every prediction
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record(st)
            call()
            e[1].record(st)
            e[2].record(st)
            est.correct(T_meas)
            e[3].record(st)
            e[3].synchronize()
            if k >= a.warmup:
                t.setdefault(name, []).append(e[0].elapsed_time(e[1]))
                t.setdefault("correct", []).append(e[2].elapsed_time(e[3]))
    s = est.state()
    assert s.status == 0 and s.predict_status == 0, (s.status, s.predict_status)
    ms, _, _, _ = timed_frames(ndt, dscans, T_init, a.warmup, a.frames)
    t["ndt_submit"] = ms
    for name, v in t.items():
        out[name + "_ms"] = stats(v)
        print(f"{name:22s} median {out[name + '_ms']['median']:.4f} ms (min {min(v):.4f} max {max(v):.4f})", flush=True)
    loops = {m: make_loop(m) for m in ("none", "device", "host")}
    t_loop, flagged = {m: [] for m in loops}, {m: 0 for m in loops}
    for k in range(a.warmup + a.frames):
        for m, loop in loops.items():                                # alternating: all three see the same machine state
            sc = scans[k % len(scans)]
            t0 = time.perf_counter()
            step = loop.step(sc) if m == "none" else loop.step(sc, dt=0.1)
            if k >= a.warmup:
                t_loop[m].append((time.perf_counter() - t0) * 1e3)
                flagged[m] += step.flagged
    for m in loops:
        out[f"loop_{m}_ms"] = stats(t_loop[m])
        out[f"loop_{m}_flagged"] = int(flagged[m])
        print(f"LocalisationLoop(sps_cvm, ndt), estimator {m:6s} median {out[f'loop_{m}_ms']['median']:.3f} ms per frame "
              f"(min {min(t_loop[m]):.3f} max {max(t_loop[m]):.3f}; {flagged[m]} flagged)", flush=True)
    print(json.dumps(out))


def ndt_c2f_main(a, scans, dscans, mp, T_init):
    """--coarse-to-fine: see the module docstring.  The sensor stands still at I, so the estimator runs with zero velocity
    and a 0.1 s scan period, as in --estimator."""
    from sps_amd.pose_estimator import PoseEstimator
    res = tuple(float(v) for v in a.resolutions.split(","))
    L = len(res)
    map64 = mp[:, :3].astype(np.float64)
    st = torch.cuda.current_stream()
    I4 = np.eye(4)

    def stats(v):
        return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    def alternate(calls):
        """hipEvent time around every call of ``calls`` (name -> function of the frame's scan that returns a pending object),
        alternating frame by frame -> name -> (ms per frame, the last result)"""
        t, last = {n: [] for n in calls}, {}
        for k in range(a.warmup + a.frames):
            s = dscans[k % len(dscans)]
            for n, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                pend = call(s)
                e1.record(st)
                last[n] = pend.result()
                e1.synchronize()
                if k >= a.warmup:
                    t[n].append(e0.elapsed_time(e1))
        return t, last

    out = {"frames": a.frames, "warmup": a.warmup, "n_map": len(mp), "resolutions": res}
    for budget, cap in ((30, 10), (90, 30)):
        pyr = NDTLocaliser(map64, resolutions=res, iterations=budget, level_iterations=(cap,) * L)
        T_dev = torch.from_numpy(np.ascontiguousarray(T_init)).cuda()
        t, last = alternate({"submit": lambda s: pyr.submit(s, len(s), T_init),
                             "from_device": lambda s: pyr.submit_from_device(s, len(s), T_dev, coarse_to_fine=True)})
        assert last["submit"].pose.tobytes() == last["from_device"].results[0].pose.tobytes()
        out[f"k1_budget{budget}"] = {n: stats(v) for n, v in t.items()}
        print(f"budget {budget} K = 1: submit on the pyramid median {np.median(t['submit']):.3f} ms, submit_from_device("
              f"coarse_to_fine) {np.median(t['from_device']):.3f} ms ({last['submit'].iterations} slots)", flush=True)
        for K in (8, 64):
            starts = hypothesis_starts(T_init, K)
            t, last = alternate({"single_map": lambda s: pyr.submit_batch(s, len(s), starts, iterations=30),
                                 "coarse_to_fine": lambda s: pyr.submit_batch(s, len(s), starts, coarse_to_fine=True)})
            rows = {n: dict(stats(v), best=r.best, slots_max=max(p.iterations for p in r.results),
                            error_m=round(LR.pose_difference(r.pose, I4)[0], 5)) for (n, v), r in zip(t.items(), last.values())}
            out[f"k{K}_budget{budget}"] = rows
            print(f"budget {budget} K = {K}: single-map batch (30 iterations) median {rows['single_map']['median']:.3f} ms, error "
                  f"{rows['single_map']['error_m']:.4f} m; coarse to fine median {rows['coarse_to_fine']['median']:.3f} ms, longest "
                  f"hypothesis {rows['coarse_to_fine']['slots_max']} slots, error {rows['coarse_to_fine']['error_m']:.4f} m", flush=True)
    # the loop per frame, host wall clock: the UKF on the pyramid on the device path and on the host path; then all queued on
    # an online pyramid with update and carve
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(mp)
    pyr = NDTLocaliser(map64, resolutions=res, iterations=30, level_iterations=(10,) * L)
    caps = tuple(max(2 * len(np.unique(np.floor(map64 / r).astype(np.int64), axis=0)), 4096) for r in res)
    online = NDTLocaliser(map64, resolutions=res, iterations=30, level_iterations=(10,) * L, level_capacities=caps,
                          capacity=1 << 16)

    def make_loop(loc, device_guess, **kw):
        return LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=VS, epsilon=EPS), loc, I4, estimator=PoseEstimator(I4, "cuda"),
                                device_guess=device_guess, coarse_to_fine=True, **kw)
    loops = {"pyramid_device": make_loop(pyr, True), "pyramid_host": make_loop(pyr, False),
             "online_device": make_loop(online, True, update_map=True, carve_map=True),
             "online_host": make_loop(online, False, update_map=True, carve_map=True)}
    t_loop, flagged = {m: [] for m in loops}, {m: 0 for m in loops}
    for k in range(a.warmup + a.frames):
        for m, loop in loops.items():                                # alternating: all see the same machine state
            t0 = time.perf_counter()
            step = loop.step(scans[k % len(scans)], dt=0.1)
            if k >= a.warmup:
                t_loop[m].append((time.perf_counter() - t0) * 1e3)
                flagged[m] += step.flagged
    for m in loops:
        out[f"loop_{m}_ms"] = stats(t_loop[m])
        out[f"loop_{m}_flagged"] = int(flagged[m])
        print(f"LocalisationLoop(sps_cvm, pyramid, ukf, coarse_to_fine) {m:15s} median {out[f'loop_{m}_ms']['median']:.3f} ms per "
              f"frame (min {min(t_loop[m]):.3f} max {max(t_loop[m]):.3f}; {flagged[m]} flagged)", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
