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
from sps_amd.localiser import LocalisationLoop, ScanToMapLocaliser  # noqa: E402
from sps_amd.sps_filters import SPSCVMFilter, SPSFilter  # noqa: E402
from tests import localiser_reference as LR  # noqa: E402
from tests.helpers import CFG, net_from_params  # noqa: E402

VS, EPS = CFG["MODEL"]["VOXEL_SIZE"], CFG["FILTER"]["THRESHOLD"]


def restatement_only(a):
    mp = synthetic.build_map()
    index = LR.MapIndex(mp, 1.0)
    T_init = LR.perturbation(0.15, 0.12, 0.05, 1.0)
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
    a = ap.parse_args()
    if a.cpu_only:
        return restatement_only(a)
    assert torch.cuda.is_available(), "localiser_timing needs the MI355X"
    scans = [synthetic.lidar_scan(seed=40 + i, n_beams=64, n_azimuth=1750) for i in range(12)]   # world frame = sensor at I
    dscans = [torch.from_numpy(s).cuda() for s in scans]
    mp = synthetic.build_map()
    loc = ScanToMapLocaliser(mp[:, :3])
    T_init = LR.perturbation(0.15, 0.12, 0.05, 1.0)

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


if __name__ == "__main__":
    main()
