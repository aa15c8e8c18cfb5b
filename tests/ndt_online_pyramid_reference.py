"""Numpy restatement of the online NDT pyramid (include/sps_hip.h, "NDT localiser, online pyramid").  Nothing
new is computed here: a level is the single online map of its resolution and capacity, so this file only composes the
existing restatements, tests/ndt_update_reference.py's ``build`` / ``update`` and tests/ndt_carve_reference.py's ``carve`` once
per level, and tests/ndt_pyramid_reference.py's ``align`` over the levels' current cell maps.  It shares no code with
sps_amd/localiser.py and never touches the native library."""
import numpy as np

from tests import ndt_carve_reference as CR
from tests import ndt_pyramid_reference as PR
from tests import ndt_update_reference as UR


def build(map_xyz, resolutions, capacities, min_points=6, eig_ratio=0.01):
    """the dynamic maps of the levels after sps_ndt_pyramid_build_dynamic, coarsest first"""
    assert len(resolutions) == len(capacities)
    return [UR.build(map_xyz, c, r, min_points, eig_ratio) for r, c in zip(resolutions, capacities)]


def update(levels, pts, T, **kw):
    """sps_ndt_pyramid_update: UR.update on every level; the info words of every level, coarsest first"""
    return [UR.update(m, pts, T, **kw) for m in levels]


def margins(levels, end_margin=None):
    """one end margin per level from None (each level's resolution), one value for all levels or one value per level"""
    if end_margin is None:
        return [m["resolution"] for m in levels]
    if np.ndim(end_margin) == 0:
        return [float(end_margin)] * len(levels)
    assert len(end_margin) == len(levels)
    return [float(v) for v in end_margin]


def carve(levels, pts, T, end_margin=None, visited=None, **kw):
    """sps_ndt_pyramid_carve: CR.carve on every level; the info words of every level.  ``visited`` (a list): gets one list
    per level with the number of cells every cast ray visited there."""
    out = []
    for m, em in zip(levels, margins(levels, end_margin)):
        v = None if visited is None else []
        out.append(CR.carve(m, pts, T, end_margin=em, visited=v, **kw))
        if visited is not None:
            visited.append(v)
    return out


def cmaps(levels):
    """the levels' current cell maps in the form the alignment's restatement reads"""
    return [UR.as_cmap(m) for m in levels]


def align(pts, levels, T_init, **kw):
    """sps_ndt_pyramid_align on the levels as they are now"""
    return PR.align(pts, cmaps(levels), T_init, **kw)
