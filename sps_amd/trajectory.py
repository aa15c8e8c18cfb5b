"""Trajectory scoring and storage for the localisation experiment: what the reference does with ``evo_ape`` on the
recorded poses (exp_pipeline/loc_exp_general.bash), without evo."""
from __future__ import annotations

import numpy as np


def _stack(poses) -> np.ndarray:
    a = np.asarray(poses, dtype=np.float64)
    if a.ndim != 3 or a.shape[1] < 3 or a.shape[2] != 4:
        raise ValueError(f"poses must be [n, 4, 4] (or [n, 3, 4]), got {a.shape}")
    return a


def ape_translation(est, ref) -> dict:
    """The statistic ``evo_ape`` prints by default (pose relation "translation part", no alignment, no scale
    correction): e_i = || t_est,i - t_ref,i ||, reported as rmse, mean, median, std, min, max (std is the population
    standard deviation, as numpy's and evo's)."""
    e, r = _stack(est), _stack(ref)
    if len(e) != len(r):
        raise ValueError(f"trajectories differ in length: {len(e)} vs {len(r)}")
    if len(e) == 0:
        raise ValueError("empty trajectory")
    err = np.linalg.norm(e[:, :3, 3] - r[:, :3, 3], axis=1)
    return {"rmse": float(np.sqrt(np.mean(err * err))), "mean": float(np.mean(err)), "median": float(np.median(err)),
            "std": float(np.std(err)), "min": float(np.min(err)), "max": float(np.max(err))}


def rotation_angle(A, B) -> float:
    """Angle (radians) of the relative rotation between two poses."""
    R = np.asarray(A, dtype=np.float64)[:3, :3].T @ np.asarray(B, dtype=np.float64)[:3, :3]
    s = np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    return float(np.arctan2(s, (np.trace(R) - 1.0) / 2.0))


def write_trajectory(path, stamps, poses) -> None:
    """One line per frame: the stamp, then the 12 entries of the top three rows of the pose, row-major, blank
    separated; floats in repr precision, so read_trajectory returns the same bits."""
    p = _stack(poses) if len(poses) else np.zeros((0, 4, 4))
    if len(p) != len(stamps):
        raise ValueError("one stamp per pose")
    with open(path, "w") as f:
        for s, T in zip(stamps, p):
            f.write(" ".join([str(s)] + [repr(float(v)) for v in T[:3].reshape(-1)]) + "\n")


def read_trajectory(path):
    """(stamps as written, poses [n, 4, 4]) of a file written by write_trajectory."""
    stamps, poses = [], []
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w:
                continue
            if len(w) != 13:
                raise ValueError(f"{path}: expected a stamp and 12 numbers, got {len(w)} fields")
            T = np.eye(4)
            T[:3] = np.array([float(v) for v in w[1:]]).reshape(3, 4)
            stamps.append(w[0])
            poses.append(T)
    return stamps, np.array(poses).reshape(-1, 4, 4)
