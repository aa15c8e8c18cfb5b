#!/usr/bin/env python3
"""Capture the constant-velocity pose predictions of the REFERENCE's second SPS node
(c_ws/src/sps_filter/scripts/sps_node_cvm.py:87-109, SPS.get_prediction_model) for seeded rigid-motion pose lists.

The node module is imported with the stubs of tools/capture_goldens.py (plus the ROS message packages it names) and
``SPS.get_prediction_model`` is called unbound on a ``SimpleNamespace(poses=...)``: nothing of ROS executes.  Runs ONLY
where the reference is checked out; writes tests/golden/cvm_poses.npz (arrays only):
``poses_<n>`` [n, 4, 4] -- the list as the node holds it, the leading identity included -- and ``pred_<n>`` [4, 4].
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from capture_goldens import OUT, REF, install_stubs  # noqa: E402

NODE = os.path.join(os.path.dirname(REF), "c_ws", "src", "sps_filter", "scripts", "sps_node_cvm.py")
LENGTHS = (1, 3, 4, 10, 11, 25)


def rigid(rng, scale=1.0):
    """A random rigid motion: rotation about a random axis by up to ~0.2 rad, translation up to ~scale metres."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-0.2, 0.2)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    T[:3, 3] = rng.uniform(-scale, scale, size=3)
    return T


def pose_list(rng, n):
    """[I, P1, P2, ...]: what the node holds after n - 1 odometry messages of a moving platform."""
    poses = [np.eye(4)]
    cur = rigid(rng, 20.0)
    for _ in range(n - 1):
        cur = cur @ rigid(rng, 0.6)
        poses.append(cur.copy())
    return poses


def main():
    install_stubs()
    for name, attrs in (("std_msgs", {}), ("std_msgs.msg", {"Float32": object}), ("nav_msgs", {}),
                        ("nav_msgs.msg", {"Odometry": object}), ("geometry_msgs", {}), ("geometry_msgs.msg", {})):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("sps_node_cvm_ref", NODE)
    node = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(node)
    rng = np.random.default_rng(20240607)
    out = {"lengths": np.array(LENGTHS)}
    for n in LENGTHS:
        poses = pose_list(rng, n)
        out[f"poses_{n}"] = np.stack(poses)
        out[f"pred_{n}"] = np.array(node.SPS.get_prediction_model(types.SimpleNamespace(poses=[p.copy() for p in poses])))
    np.savez(os.path.join(OUT, "cvm_poses.npz"), **out)
    print("wrote cvm_poses.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
