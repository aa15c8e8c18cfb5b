#!/usr/bin/env python3
"""Per-frame latency of the online SPS filter on one MI355X at config-2 size (64 x 1750 rays, ~100 k points, the
synthetic.build_map() map, voxel 0.1), three paths in the same process on the same scans and weights:

  stable   pipeline.StableFilter as it stands: scores + the three kept columns
  sps      sps_filters.SPSFilter with every output on: whole kept rows, labels, both debug clouds, metric sums
  eager    the node-shaped loop: StableFilter for the device part, then what sps_node.py:123-161 does with the scores on
           the host -- MSELoss / R2 in torch, .cpu(), np.where, calculate_metrics, scan[mask], np.hstack for the two clouds

A frame is timed with the host wall clock around submit -> result (or the whole eager callback), which ends in a device
synchronisation either way.  The three paths are interleaved round by round (--rounds rounds of --frames frames each after
--warmup frames) so that drift hits them alike; per path the median of each round is taken and the spread of those
medians reported, the way profiles/round6_b/repeatability.txt states spread.  Prints one line per path and a JSON line.

    python tools/sps_filter_timing.py [--frames 100] [--rounds 5] [--warmup 20] [--one-frame]

``--one-frame`` runs a warm-up and ONE SPSFilter frame: the target of a ``rocprofv3 --kernel-trace --stats`` run.
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
from sps_amd.datasets import util  # noqa: E402
from sps_amd.pipeline import StableFilter  # noqa: E402
from sps_amd.sps_filters import SPSFilter  # noqa: E402
from tests.helpers import CFG, net_from_params  # noqa: E402

VS, EPS = CFG["MODEL"]["VOXEL_SIZE"], CFG["FILTER"]["THRESHOLD"]


def pose(k):
    a = 0.01 * k
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = [0.05 * (k % 40), 0.02 * (k % 40), 0.0]
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--one-frame", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sps_filter_timing needs the MI355X"
    scans = [synthetic.lidar_scan(seed=40 + i, n_beams=64, n_azimuth=1750) for i in range(12)]   # (x, y, z, label) float32
    mp = torch.from_numpy(synthetic.build_map())
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    stable = StableFilter(net, mp, voxel_size=VS, epsilon=EPS)
    sps = SPSFilter(net, mp, voxel_size=VS, epsilon=EPS)
    loss_fn = torch.nn.MSELoss().cuda()

    def run_stable(k):
        return stable(scans[k % len(scans)], pose(k))

    def run_sps(k):
        return sps(scans[k % len(scans)], pose(k))

    def run_eager(k):
        scan, T = scans[k % len(scans)], pose(k)
        scan_tr = util.transform_point_cloud(scan[:, :3], T)                       # the node's own host transform (:103)
        labels = torch.tensor(scan[:, 3], dtype=torch.float32).reshape(-1, 1).cuda()
        pend = stable.submit(scan, T)
        r = pend.result()
        s = r.scores
        loss = loss_fn(s.view(-1), labels.view(-1))
        r2 = net.r2score(s.view(-1), labels.view(-1))
        s = s.cpu()
        pred = np.where(s.view(-1) < EPS, 0, 1)
        gt = np.where(labels.cpu().view(-1) < EPS, 0, 1)
        m = util.calculate_metrics(gt, pred)
        filtered = scan[(s <= EPS)]
        cloud = np.hstack([scan_tr[:, :3], pred.reshape(-1, 1)])
        n = len(scan)
        submap_points = pend._batch[n:n + r.n_submap_voxels, 1:4].cpu()            # :157 (StableFilter keeps them on the device)
        sub = torch.hstack([submap_points, torch.ones(submap_points.shape[0], 1)])
        return float(loss), float(r2), m, len(filtered), cloud.shape, sub.shape

    paths = {"stable": run_stable, "sps": run_sps, "eager": run_eager}
    for k in range(a.warmup):
        for fn in paths.values():
            fn(k)
    torch.cuda.synchronize()
    if a.one_frame:
        r = run_sps(a.warmup)
        print(json.dumps({"one_frame": True, "n": len(r.scores), "kept": len(r.filtered), "M": r.n_submap_voxels}))
        return
    med = {name: [] for name in paths}
    stages = []
    k = a.warmup
    for _ in range(a.rounds):
        for name, fn in paths.items():
            t = []
            for i in range(a.frames):
                t0 = time.perf_counter()
                r = fn(k + i)
                t.append(time.perf_counter() - t0)
                if name == "sps":
                    stages.append((r.t_prune, r.t_infer, r.t_finish))
            med[name].append(float(np.median(t)) * 1e3)
        k += a.frames
    out = {"n_scan": int(np.mean([len(s) for s in scans])), "n_map": len(mp), "frames": a.frames, "rounds": a.rounds,
           "warmup": a.warmup}
    for name, v in med.items():
        mid, lo, hi = float(np.median(v)), min(v), max(v)
        print(f"{name:7s} median of round medians {mid:7.3f} ms   rounds min {lo:7.3f} max {hi:7.3f}   "
              f"spread {100 * (hi - lo) / mid:5.2f} %", flush=True)
        out[name] = {"ms": round(mid, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "round_medians_ms": [round(x, 4) for x in v]}
    out["sps_gpu_stages_ms"] = [round(float(np.median([s[i] for s in stages])) * 1e3, 4) for i in range(3)]
    print(f"sps GPU stages (prune, infer, finish) {out['sps_gpu_stages_ms']} ms")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
