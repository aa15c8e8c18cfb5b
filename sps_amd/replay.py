"""Replay a recorded sequence through an online filter: the file side of the reference's scan publisher
(c_ws/src/scans_pub/scripts/pub_scans.py:34-70) without ROS.

    $DATA/sequence/SEQ/scans/<stamp>.npy      rows (x, y, z, label) in the sensor frame
    $DATA/sequence/SEQ/poses/<stamp>.txt      4x4, comma separated
    $DATA/sequence/SEQ/map_transform          4x4, comma separated

A scan reaches the map frame through ``map_transform @ pose`` (pub_scans.py:69-70 applies the pose, then the map
transform); the filters take that product as the frame's pose.
"""
from __future__ import annotations

import os

import numpy as np


def _by_stamp(names):
    return sorted(names, key=lambda f: (float(os.path.splitext(f)[0]), f))


class ScanReplay:
    """Iterates ``(stamp, scan_rows, pose, map_transform)`` over a sequence; ``stamp`` is the file stem, as
    pub_scans.py:64 takes it.

    Files are ordered by the FLOAT VALUE of their stem.  The reference orders them with ``sorted(os.listdir(...))``
    (pub_scans.py:84-90), a string sort: the two agree whenever the names have equal length (the recorded sequences:
    ten integer digits, a dot, six decimals) and differ otherwise -- "10.5.npy" sorts before "9.5.npy" as a string and
    after it here, which is the order the scans were taken in."""

    def __init__(self, data_dir, seq):
        root = os.path.join(str(data_dir), "sequence", str(seq))
        self.scans_pth = os.path.join(root, "scans")
        self.poses_pth = os.path.join(root, "poses")
        self.scans = _by_stamp(os.listdir(self.scans_pth))
        self.poses = _by_stamp(os.listdir(self.poses_pth))
        self.map_transform = np.loadtxt(os.path.join(root, "map_transform"), delimiter=",")
        assert len(self.scans) == len(self.poses), 'Must have the same length!!'          # pub_scans.py:54

    def __len__(self):
        return len(self.scans)

    def __iter__(self):
        for scan, pose in zip(self.scans, self.poses):
            stamp = os.path.splitext(scan)[0]
            scan_data = np.load(os.path.join(self.scans_pth, scan))
            pose_data = np.loadtxt(os.path.join(self.poses_pth, pose), delimiter=",")
            yield stamp, scan_data, pose_data, self.map_transform


def write_synthetic_tree(root, n_scans: int, seq: str = "synthetic", n_azimuth: int = 400, n_beams: int = 32, step: float = 0.5):
    """A $DATA tree in the reference's on-disk layout from sps_amd.synthetic: ``n_scans`` scans of a sensor that advances
    ``step`` m per scan along x and turns slowly, stored in the sensor frame, plus maps/base_map.asc.npy.  Returns the
    map [M, 4]."""
    from . import synthetic
    kw = dict(n_azimuth=n_azimuth, n_beams=n_beams)
    seq_dir = os.path.join(str(root), "sequence", seq)
    for d in (os.path.join(str(root), "maps"), os.path.join(seq_dir, "scans"), os.path.join(seq_dir, "poses")):
        os.makedirs(d, exist_ok=True)
    pc_map = synthetic.sequence_map(n_scans, step, **kw)
    np.save(os.path.join(str(root), "maps", "base_map.asc.npy"), pc_map)
    ang = 0.3
    T_map = np.array([[np.cos(ang), -np.sin(ang), 0, 0.5], [np.sin(ang), np.cos(ang), 0, -0.25], [0, 0, 1, 0.1], [0, 0, 0, 1.0]])
    np.savetxt(os.path.join(seq_dir, "map_transform"), T_map, delimiter=",")
    for i in range(n_scans):
        world = synthetic.lidar_scan(100 + i, x_offset=step * i, **kw)
        a = 0.02 * i
        T = np.eye(4)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[:3, 3] = [step * i, 0.0, 0.0]
        pose = np.linalg.inv(T_map) @ T                                           # map_transform @ pose = T
        sensor = (np.linalg.inv(T) @ np.c_[world[:, :3].astype(np.float64), np.ones(len(world))].T).T[:, :3]
        stamp = f"{1656500000.0 + 0.5 * i:.6f}"
        np.save(os.path.join(seq_dir, "scans", stamp + ".npy"), np.c_[sensor, world[:, 3]].astype(np.float32))
        np.savetxt(os.path.join(seq_dir, "poses", stamp + ".txt"), pose, delimiter=",")
    return pc_map
