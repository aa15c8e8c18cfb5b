#!/usr/bin/env python3
"""One SHA-256 per output buffer of every entry point of the localisers, on the seeded scenes of tools/localiser_timing.py at a reduced
size (32 x 400 rays, the 57 k-point map: ~2.5 k cells, ~4 k points after thinning at 0.4 m).  For comparing two builds of
the library on one machine and one ROCm release:

    SPS_LIB=/path/to/the/other/libsps_hip.so python tools/ndt_digest.py > a.txt
    python tools/ndt_digest.py > b.txt && diff a.txt b.txt

The raw host buffers are hashed, not the parsed results, so every word the device wrote counts; of a LocalisationLoop,
the stacked poses of 8 steps around a filter that keeps every row.  Only the public API and the pending objects' ``_host``
are used, so the file also runs on an older tree against the same library (``SPS_LIB``), which compares two wrappers.
The digests hold the device exp of one ROCm release: they are not golden values and belong in no test.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from localiser_timing import hypothesis_starts, search_poses  # noqa: E402
from sps_amd import synthetic  # noqa: E402
from sps_amd.localiser import LocalisationLoop, NDTLocaliser, ScanToMapLocaliser, pose_grid  # noqa: E402
from sps_amd.pose_estimator import PoseEstimator  # noqa: E402
from tests import localiser_reference as LR  # noqa: E402

SIZE = dict(n_beams=32, n_azimuth=400)
LEAF = 0.4


def digest(name, *arrays):
    for i, a in enumerate(arrays):
        a = np.ascontiguousarray(a)
        tag = name if len(arrays) == 1 else f"{name}[{i}]"
        print(f"{tag:28s} {a.dtype!s:8s} {a.size:8d}  {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


class KeepAll:
    """A filter that takes no pose and keeps every row.  ``device_rows``: its pending frame exposes the rows and their
    count on the device, as SPSFilter's does, so the loop registers before the frame's result()."""
    takes_pose = False

    def __init__(self, device_rows):
        self.device_rows = device_rows

    def submit(self, scan):
        return KeptFrame(scan, self.device_rows)


class KeptFrame:
    def __init__(self, rows, device_rows):
        self.filtered = rows
        if device_rows:
            self._filtered = rows
            self.count_dev = torch.full((1,), len(rows), dtype=torch.int32, device=rows.device)

    def result(self):
        return self


def source_arrays(cells):
    """the arrays of NDTLocaliser.source_cells in a fixed order"""
    return [cells[k] for k in ("mean", "cov", "count", "valid")]


def loops(ndt, T_init):
    """the stacked poses of 8 steps in four set-ups, with the rows on the device and fetched"""
    scans = [torch.from_numpy(synthetic.lidar_scan(seed=40 + k, **SIZE)).cuda() for k in range(8)]
    setups = (("plain", lambda: {}),
              ("5 hypotheses", lambda: dict(hypotheses=pose_grid([0.0, -0.5, 0.5], 0.0, [0.0, 5.0])[:5])),
              ("search 75 keep 4", lambda: dict(search=pose_grid(np.linspace(-1.0, 1.0, 5), np.linspace(-0.5, 0.5, 3),
                                                                 np.linspace(-4.0, 4.0, 5))[[37] + list(range(37)) + list(range(38, 75))],
                                                search_keep=4)),
              ("device_guess", lambda: dict(estimator=PoseEstimator(T_init, "cuda"), device_guess=True)))
    for name, kw in setups:
        for device_rows in (True, False):
            loop = LocalisationLoop(KeepAll(device_rows), ndt, T_init, **kw())
            steps = [loop.step(s, **(dict(dt=0.1) if name == "device_guess" else {})) for s in scans]
            digest(f"loop {name} {'dev' if device_rows else 'host'}", np.stack(loop.poses))
            print(f"# loop {name}: flagged {[int(s.flagged) for s in steps]}", flush=True)


def main():
    assert torch.cuda.is_available(), "ndt_digest needs the MI355X"
    scan = torch.from_numpy(synthetic.lidar_scan(seed=40, **SIZE)).cuda()    # world frame = sensor at I
    other = torch.from_numpy(synthetic.lidar_scan(seed=41, x_offset=6.0, **SIZE)).cuda()   # 6 m on: existing and new cells
    map64 = synthetic.build_map(**SIZE)[:, :3].astype(np.float64)
    T_init = LR.perturbation(0.15, 0.12, 0.05, 1.0)
    static = NDTLocaliser(map64, leaf=LEAF)
    dyn = NDTLocaliser(map64, leaf=LEAF, cell_capacity=2 * static.n_cells)
    n = len(scan)
    digest("static map_cells", *static.map_cells())
    digest("dynamic map_cells", *dyn.map_cells())
    pend = static.submit(scan, n, T_init, with_normal=True)
    pend.result()
    digest("submit with_normal", pend._host.numpy())
    pend = static.submit_batch(scan, n, hypothesis_starts(T_init, 5))
    pend.result()
    digest("submit_batch K=5", pend._host.numpy())
    pend = static.score_poses(scan, n, search_poses(T_init, 75))
    pend.result()
    digest("score_poses P=75", pend._host.numpy())
    pend = static.relocalise(scan, n, search_poses(T_init, 75), keep=4)
    pend.result()
    digest("relocalise keep=4", pend._batch._host.numpy())
    pend = dyn.integrate(other, len(other), np.eye(4))
    r = pend.result()
    digest("integrate", pend._host.numpy())
    digest("map_cells after integrate", *dyn.map_cells())
    print(f"# {static.n_cells} cells, integrate: {r}", flush=True)
    pend = ScanToMapLocaliser(map64, leaf=LEAF).submit(scan, n, T_init, with_normal=True)
    pend.result()
    digest("icp submit with_normal", pend._host.numpy())
    pend = dyn.submit(scan, n, T_init, integrate=True, carve=True)
    r = pend.result()
    digest("submit integrate carve", pend._host.numpy())
    pend = dyn.carve(other, len(other), np.eye(4))
    print(f"# combined: {r.map_update} {r.map_carve}, carve: {pend.result()}", flush=True)
    digest("carve", pend._host.numpy())
    digest("map_cells after carve", *dyn.map_cells(), *dyn.carve_state())
    pyr = NDTLocaliser(map64, leaf=LEAF, resolutions=(2.0, 1.0, 0.5))
    pend = pyr.submit(scan, n, T_init, with_normal=True)
    pend.result()
    digest("pyramid submit", pend._host.numpy())
    online = NDTLocaliser(map64, leaf=LEAF, resolutions=(2.0, 1.0, 0.5), level_capacities=[2 * c for c in pyr.level_cells])
    for name, pend in (("online pyramid submit", online.submit(scan, n, T_init, with_normal=True)),
                       ("online pyramid integrate", online.integrate(other, len(other), np.eye(4))),
                       ("online pyramid carve", online.carve(other, len(other), np.eye(4))),
                       ("online pyramid combined", online.submit(scan, n, T_init, integrate=True, carve=True))):
        pend.result()
        digest(name, pend._host.numpy())
    for l in range(3):
        digest(f"online pyramid level {l}", *online.pyramid_cells(l), *online.carve_state(l))
    cells = NDTLocaliser(map64, leaf=LEAF, source="cells")
    pend = cells.submit(scan, n, T_init, with_normal=True)
    r = pend.result()
    digest("cells submit with_normal", pend._host.numpy())
    print(f"# source cells: {r.n_sources} valid, status {r.status} after {r.iterations}", flush=True)
    pend = cells.submit_batch(scan, n, hypothesis_starts(T_init, 5), d2d=True)
    pend.result()
    digest("cells submit_batch K=5", pend._host.numpy())
    pend = cells.score_poses(scan, n, search_poses(T_init, 75), d2d=True)
    pend.result()
    digest("cells score_poses P=75", pend._host.numpy())
    pend = cells.relocalise(scan, n, search_poses(T_init, 75), keep=4, d2d=True)
    pend.result()
    digest("cells relocalise keep=4", pend._batch._host.numpy())
    digest("source_cells", *source_arrays(cells.source_cells(scan, n)))
    cpyr = NDTLocaliser(map64, leaf=LEAF, resolutions=(2.0, 1.0, 0.5), source="cells", source_resolutions=(2.0, 1.0, 0.5),
                        source_min_points=6, iterations=90, level_iterations=(30, 30, 30))
    pend = cpyr.submit(scan, n, T_init, with_normal=True)
    r = pend.result()
    digest("cells pyramid submit", pend._host.numpy())
    print(f"# cells pyramid: status {r.status} after {r.iterations}", flush=True)
    for l in range(3):
        digest(f"source_cells level {l}", *source_arrays(cpyr.source_cells(scan, n, level=l)))
    pend = static.submit_from_device(scan, n, torch.from_numpy(np.ascontiguousarray(T_init)).cuda())
    pend.result()
    digest("submit_from_device", pend._host.numpy())
    loops(static, T_init)


if __name__ == "__main__":
    main()
