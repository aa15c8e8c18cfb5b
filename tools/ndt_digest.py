#!/usr/bin/env python3
"""One SHA-256 per output buffer of every NDT entry point, on the seeded scenes of tools/localiser_timing.py at a reduced
size (32 x 400 rays, the 57 k-point map: ~2.5 k cells, ~4 k points after thinning at 0.4 m).  For comparing two builds of
the library on one machine and one ROCm release:

    SPS_LIB=/path/to/the/other/libsps_hip.so python tools/ndt_digest.py > a.txt
    python tools/ndt_digest.py > b.txt && diff a.txt b.txt

The raw host buffers are hashed, not the parsed results, so every word the device wrote counts.  The digests hold the
device exp of one ROCm release: they are not golden values and belong in no test.
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
from sps_amd.localiser import NDTLocaliser  # noqa: E402
from tests import localiser_reference as LR  # noqa: E402

SIZE = dict(n_beams=32, n_azimuth=400)
LEAF = 0.4


def digest(name, *arrays):
    for i, a in enumerate(arrays):
        a = np.ascontiguousarray(a)
        tag = name if len(arrays) == 1 else f"{name}[{i}]"
        print(f"{tag:28s} {a.dtype!s:8s} {a.size:8d}  {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


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


if __name__ == "__main__":
    main()
