"""Numpy restatements of the reference node steps the online baseline filters replace (tests only)."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def crop_indices(points, centre, radius=30.0):
    """mapmos_node.py:63-68 select_points_within_radius, as written there (float64 distances, np.where order)."""
    distances = np.sqrt(np.sum((points - centre) ** 2, axis=1))
    return np.where(distances <= radius)[0]


def crop_golden():
    """tests/golden/mapmos_crop.npz (tools/capture_baseline_goldens.py): {dtype tag: (map, [indices per pose])}, poses."""
    z = np.load(os.path.join(GOLD, "mapmos_crop.npz"))
    out = {}
    for tag in ("64", "32"):
        off = z["off" + tag]
        out[tag] = (z["map" + tag], [z["sel" + tag][off[i]:off[i + 1]] for i in range(len(off) - 1)])
    return out, z["poses"], float(z["radius"])


def mos4d_window_rows(transformed, indices):
    """mos4d_node.py:97-116: hstack(scan_tr, index) per scan, np.vstack of the window, .to(float32), batch column 0."""
    merged = np.vstack([np.hstack([t, np.ones((len(t), 1)) * i]) for t, i in zip(transformed, indices)])
    merged = merged.astype(np.float32)
    return np.hstack([np.zeros((len(merged), 1), np.float32), merged])
