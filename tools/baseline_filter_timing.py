#!/usr/bin/env python3
"""Per-frame latency of the online 4DMOS / MapMOS / mask filters (sps_amd/baseline_filters.py) on one MI355X at deployed
sizes, each next to a node-shaped eager loop in the same process (the reference callbacks' host steps around the same
device model):

  4DMOS   10-scan window of config-2-size scans (64 x 1750 rays, ~100 k points), voxel 0.2.
          eager: numpy transform, hstack index, list window, np.vstack, H2D, MOS4DNet.forward, (logits > 0).cpu(),
          numpy filter + calculate_metrics (mos4d_node.py:80-147)
  MapMOS  one config-2-size scan + the 30 m crop of synthetic.build_map(), voxel 0.1.
          eager: numpy radius crop of the whole map, numpy transform, two H2D, MapMOSNet.predict, to_label(..).cpu(),
          numpy filter (mapmos_node.py:70-112)
  mask    the StableFilter map (synthetic.build_map()), voxel 0.1.
          eager: numpy transform, H2D, to_coords_features + util.prune, .cpu(), numpy inverse transform (mask.py:86-147)

A frame is timed with the host wall clock around submit -> result (the filters) or the whole callback (eager), which ends
in a device synchronisation either way; the filters' GPU stage splits come from their hipEvents.  Median over --frames
after --warmup frames.  Prints one line per (filter, path) and a JSON summary line.

    python tools/baseline_filter_timing.py [--frames 200] [--warmup 20] [--only mos4d,mapmos,mask]
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
from sps_amd.baseline_filters import MapMOSFilter, MaskFilter, MOS4DFilter  # noqa: E402
from sps_amd.datasets import util  # noqa: E402
from sps_amd.models.baselines import MapMOSNet, MOS4DNet  # noqa: E402
from tests.helpers import state_dict_from_params  # noqa: E402


def pose(k):
    a = 0.01 * k
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = [0.05 * (k % 40), 0.02 * (k % 40), 0.0]
    return T


def model(cls, vs, oc, seed):
    m = cls(vs)
    m.MinkUNet.load_state_dict(state_dict_from_params(O.random_params(seed=seed, out_channels=oc), prefix=""))
    return m.cuda().eval().freeze()


def timed(fn, frames, warmup):
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    t = []
    for k in range(warmup, warmup + frames):
        t0 = time.perf_counter()
        r = fn(k)
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, float(np.percentile(t, 90)) * 1e3, r


def run_mos4d(scans, frames, warmup):
    m = model(MOS4DNet, 0.2, 3, 4)
    f = MOS4DFilter(m, buffer_size=10)
    stages = []

    def filt(k):
        r = f(scans[k % len(scans)], pose(k))
        stages.append((r.t_prepare, r.t_infer, r.t_filter))
        return r

    buf, idx = [], [0]

    def eager(k):
        scan = scans[k % len(scans)]
        T = pose(k)
        gt = np.where(scan[:, 3] < 0.84, 0, 1)
        tr = util.transform_point_cloud(scan[:, :3], T)
        buf.append(np.hstack([tr, np.ones(len(tr)).reshape(-1, 1) * idx[0]]))
        idx[0] += 1
        if len(buf) > 10:
            buf.pop(0)
        merged = torch.from_numpy(np.vstack(buf)).squeeze().to(torch.float32).cuda()
        coords = torch.hstack([torch.zeros(len(merged)).reshape(-1, 1).type_as(merged), merged])
        lab = (m.forward(coords) > 0).int().cpu().numpy()[-len(scan):]
        kept = scan[lab == 0]
        return util.calculate_metrics(gt, lab), len(kept)

    return timed(filt, frames, warmup), timed(eager, frames, warmup), stages[warmup:]


def run_mapmos(scans, mp, frames, warmup):
    m = model(MapMOSNet, 0.1, 1, 6)
    f = MapMOSFilter(m, mp)
    stages = []

    def filt(k):
        r = f(scans[k % len(scans)], pose(k))
        stages.append((r.t_prepare, r.t_infer, r.t_filter))
        return r

    def eager(k):
        scan = scans[k % len(scans)]
        T = pose(k)
        d = np.sqrt(np.sum((mp[:, :3] - T[:3, 3]) ** 2, axis=1))
        crop = mp[np.where(d <= 30)[0]]
        tr = util.transform_point_cloud(scan[:, :3], T)
        sp = torch.tensor(tr[:, :3], dtype=torch.float32).reshape(-1, 3).cuda()
        cp = torch.tensor(crop[:, :3], dtype=torch.float32).reshape(-1, 3).cuda()
        ls, _ = m.predict(sp, cp, torch.ones(len(sp), 1).cuda(), torch.zeros(len(cp), 1).cuda())
        lab = m.to_label(ls).cpu().numpy()
        return len(scan[lab == 0]), len(crop)

    return timed(filt, frames, warmup), timed(eager, frames, warmup), stages[warmup:]


def run_mask(scans, mp, frames, warmup):
    f = MaskFilter(mp, voxel_size=0.1)
    stages = []

    def filt(k):
        r = f(scans[k % len(scans)], pose(k))
        stages.append((r.t_prune, r.t_inverse))
        return r

    mcf = util.to_coords_features(torch.from_numpy(mp[:, :3]).cuda(), 'map', ds=0.1)

    def eager(k):
        scan = scans[k % len(scans)]
        T = pose(k)
        tr = util.transform_point_cloud(scan[:, :3], T)
        sp = torch.tensor(tr[:, :3], dtype=torch.float32).reshape(-1, 3).cuda()
        sub, n_sv = util.prune(mcf, util.to_coords_features(sp, 'scan', ds=0.1), 0.1)
        sub = sub.cpu().numpy()
        out = np.hstack([sub, np.ones((len(sub), 1), np.float32)])
        out[:, :3] = util.inverse_transform_point_cloud(out[:, :3], T)
        return len(out), n_sv

    return timed(filt, frames, warmup), timed(eager, frames, warmup), stages[warmup:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="mos4d,mapmos,mask")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "baseline_filter_timing needs the MI355X"
    scans = [synthetic.lidar_scan(seed=40 + i, n_beams=64, n_azimuth=1750) for i in range(12)]   # sensor frame, (x,y,z,s)
    mp = synthetic.build_map()
    out = {"n_scan": int(np.mean([len(s) for s in scans])), "n_map": len(mp), "frames": a.frames, "warmup": a.warmup}
    for name in a.only.split(","):
        if name == "mos4d":
            (fm, f90, _), (em, e90, _), st = run_mos4d(scans, a.frames, a.warmup)
        elif name == "mapmos":
            (fm, f90, r), (em, e90, _), st = run_mapmos(scans, mp, a.frames, a.warmup)
            out["mapmos_crop_rows"] = r.n_map
        else:
            (fm, f90, _), (em, e90, _), st = run_mask(scans, mp, a.frames, a.warmup)
        gpu = [round(float(np.median([s[i] for s in st])) * 1e3, 3) for i in range(len(st[0]))]
        print(f"{name:7s} filter  median {fm:8.2f} ms  p90 {f90:8.2f} ms  gpu stages {gpu} ms", flush=True)
        print(f"{name:7s} eager   median {em:8.2f} ms  p90 {e90:8.2f} ms", flush=True)
        out[name] = {"filter_ms": round(fm, 3), "filter_p90_ms": round(f90, 3), "eager_ms": round(em, 3),
                     "eager_p90_ms": round(e90, 3), "filter_gpu_stages_ms": gpu}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
