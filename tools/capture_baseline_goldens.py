#!/usr/bin/env python3
"""Capture the golden crop of the MapMOS node from the REFERENCE python (c_ws/src/mapmos/scripts/mapmos_node.py,
``MapMos.select_points_within_radius``, mapmos_node.py:63-68) for tests/test_baseline_filters_cpu.py and
tests/test_hip_baseline_filters.py.  Runs only where the reference tree exists (its mapmos/scripts directory as the
first argument or in $MAPMOS_REFERENCE); the node module is imported with rospy, message_filters, the message types,
sps.datasets.util and the network stubbed (only the radius selection is called).  Writes tests/golden/mapmos_crop.npz
(data only):

  map64 [m, 3] float64, map32 [m', 3] float32   synthetic maps: uniform points around the poses plus points placed on
                                                the 30 m sphere of every pose and 1 ulp inside / outside it
  poses [k, 4, 4]                               the poses whose T[:3, 3] is the crop centre (mapmos_node.py:79)
  sel64, off64 / sel32, off32                   the reference's selected indices per pose, concatenated (off = [k + 1])
"""
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MAPMOS_REFERENCE", "")
if not os.path.exists(os.path.join(REF, "mapmos_node.py")):
    raise SystemExit("usage: capture_baseline_goldens.py <reference>/c_ws/src/mapmos/scripts")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
RADIUS = 30.0


def stub_ros():
    for name in ("rospy", "message_filters", "nav_msgs", "nav_msgs.msg", "sensor_msgs", "sensor_msgs.msg", "sps",
                 "sps.datasets", "sps.datasets.util", "mapmos"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["nav_msgs.msg"].Odometry = object
    sys.modules["sensor_msgs.msg"].PointCloud2 = object
    sys.modules["mapmos"].MapMOSNet = object
    sys.modules["sps"].datasets = sys.modules["sps.datasets"]
    sys.modules["sps.datasets"].util = sys.modules["sps.datasets.util"]


def poses():
    out = []
    for ang, t in ((0.0, (0.0, 0.0, 0.0)), (0.7, (1.5, -2.25, 0.5)), (-2.1, (12.75, 4.5, -1.25))):
        T = np.eye(4)
        T[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]
        T[:3, 3] = t
        out.append(T)
    return np.stack(out)


def boundary_points(centres, dtype):
    """Per centre: points at exactly 30 m along the axes and on a 3-4-5 diagonal, and their 1-ulp neighbours."""
    pts = []
    for c in centres:
        for d in ([30, 0, 0], [-30, 0, 0], [0, 30, 0], [0, 0, -30], [18, 24, 0], [0, -18, 24]):
            p = (c + np.array(d, np.float64)).astype(dtype)
            pts.append(p)
            for k in range(3):
                if d[k] != 0:
                    for toward in (np.inf, -np.inf):
                        q = p.copy()
                        q[k] = np.nextafter(q[k], dtype(toward))
                        pts.append(q)
    return np.array(pts, dtype)


def main():
    stub_ros()
    sys.path.insert(0, REF)
    import mapmos_node as ref  # noqa: E402
    select = lambda pts, c: ref.MapMos.select_points_within_radius(None, pts, c)   # noqa: E731 (self is unused)
    P = poses()
    centres = P[:, :3, 3]
    rng = np.random.default_rng(5)
    maps = {}
    for name, dtype, n in (("64", np.float64, 900), ("32", np.float32, 1500)):
        bulk = rng.uniform(-45, 55, (n, 3)).astype(dtype)
        bulk[:, 2] = rng.uniform(-4, 4, n)
        m = np.concatenate([bulk, boundary_points(centres, dtype)]).astype(dtype)
        m = m[rng.permutation(len(m))]
        sel = [select(m, c) for c in centres]
        on = [int(np.sum(np.sqrt(np.sum((m - c) ** 2, axis=1)) == RADIUS)) for c in centres]
        maps["map" + name] = m
        maps["sel" + name] = np.concatenate(sel).astype(np.int32)
        maps["off" + name] = np.cumsum([0] + [len(s) for s in sel]).astype(np.int32)
        print(f"map{name}: {len(m)} points, selected {[len(s) for s in sel]}, exactly on the sphere {on}")
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "mapmos_crop.npz"), poses=P, radius=np.float64(RADIUS), **maps)
    print("wrote", os.path.join(OUT, "mapmos_crop.npz"))


if __name__ == "__main__":
    main()
