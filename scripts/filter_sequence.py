#!/usr/bin/env python3
"""Replay one recorded sequence through one of the online scan filters and print what its ROS node would log -- the
filter side of the reference's localisation experiment (c_ws/src/sps_filter/scripts/loc_exp_general.bash runs
sps | mos4d | mapmos | lts | mask | raw over a sequence, fed by scans_pub/scripts/pub_scans.py) without ROS and, unless
``--localise`` is given, without the localiser.

    --filter sps       sps_amd.sps_filters.SPSFilter       (sps_node.py)
    --filter sps_cvm   sps_amd.sps_filters.SPSCVMFilter    (sps_node_cvm.py: add_pose gets the replayed pose of the PREVIOUS frame)
    --filter raw       the SPS filter at epsilon = 2: every point passes (how loc_exp_general.bash defines "raw")
    --filter mos4d | mapmos | mask | lts                   sps_amd.baseline_filters / sps_amd.lts_filter

Two frames are kept in flight: result() of frame i is called after submit() of frame i + 1, so the host work of a
frame overlaps the device work of the one before.  Per frame the node's lines are printed behind the frame's stamp,
then the sequence means.  ``--out DIR`` writes every filtered cloud as DIR/<stamp>.npy.  ``--synthetic N`` replays N
scans of a temporary tree built from sps_amd.synthetic (no $DATA needed); without ``-w`` the weights are a seeded
random initialisation.

``--localise`` closes the loop of the experiment (sps_amd.localiser.LocalisationLoop, seeded with the first replayed
pose): the filter's kept rows are registered against the map by a device point-to-point ICP (the stand-in for
hdl_localization; not a port of it), the corrected pose goes back into the filter, and the replayed poses only score
the result.  ``--localiser ndt`` registers with sps_amd.localiser.NDTLocaliser instead: the normal-distributions transform
hdl_localization itself runs (1 m cells, DIRECT7), still without its UKF and IMU; with ``--resolutions 2,1,0.5`` it
registers every frame coarse to fine over a pyramid of cell maps (``--level-iterations`` caps each level; a ``levels:``
line then tells the iterations per level); with ``--update-map`` / ``--carve-map`` as well the pyramid is an online one
(``--level-capacities``), every level is updated and carved in the same launches and the ``map`` / ``carve`` lines come once
per level; with ``--source cells`` it registers distribution to distribution (one Gaussian per cell of the scan against
the map's; ``--source-resolution``, ``--source-min-points``), ``n_corr`` then counts source cells and the ``loc:`` line
ends with ``| N sources``, the scan's valid cells; ``--d2d`` lets ``--hypotheses``, ``--search`` and the device path of
``--estimator ukf`` register the scan's cells too (``--d2d-pyramid``: coarse to fine on the pyramid of
``--source-resolutions``); ``--source cells --resolutions 2,1,0.5 --source-resolutions 2,1,0.5``
registers the scan's cells coarse to fine, built once per level at that level's edge (``--source-min-points`` then also
takes one value per level; the ``| N sources`` are those of the level the frame ended on).  Frames then run one at a time; behind each frame's lines comes
``loc: status iterations n_corr rmse | err_t err_r`` (metres, degrees, against the replayed pose map_tr @ pose) and at
the end the absolute pose error evo_ape prints by default.  ``--global-start`` (with ``--localiser ndt``) takes the loop's
initial pose from ``NDTLocaliser.localise_global`` on the first raw scan instead of from the sequence (``--global-resolution``,
``--global-map-z``, ``--global-scan-z``, ``--global-yaw-steps``, ``--global-levels``, ``--global-frontier``; the defaults are
the slice chosen for sps_amd.synthetic: profiles/localiser_global/README.md) and prints the selected leaf, the certificate
and the error against the sequence's first pose in ``global:`` lines.  ``--match-status [DIST[,RANGE]]`` (with ``--min-inlier-fraction F``) follows every
registration by the scan-matching status at its pose and prints it in ``match:`` lines, ``--recover-global N`` registers the frame
after N flagged ones by the global search, and ``--inject-jump FRAME,DX,DY,YAW`` kidnaps the sensor to try both.
``--traj-out FILE`` writes the estimated trajectory
(stamp + the top three rows of the pose per line).
"""
from __future__ import annotations

import math
import os
import sys
import tempfile

import click
import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sps_amd.replay import ScanReplay, write_synthetic_tree  # noqa: E402

FILTERS = ("sps", "sps_cvm", "mos4d", "mapmos", "mask", "lts", "raw")
DEFAULT_CONFIG_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "config.yaml")
RAW_EPSILON = 2.0


def build_filter(name, cfg, weights, pc_map, epsilon):
    vs = cfg["MODEL"]["VOXEL_SIZE"]
    if name in ("sps", "sps_cvm", "raw"):
        from sps_amd.models import models
        from sps_amd.sps_filters import SPSCVMFilter, SPSFilter
        cls = SPSCVMFilter if name == "sps_cvm" else SPSFilter
        eps = RAW_EPSILON if name == "raw" else epsilon
        if weights:
            return cls.from_checkpoint(cfg, weights, pc_map, epsilon=eps)
        torch.manual_seed(0)
        return cls(models.SPSNet(cfg).cuda().eval().freeze(), pc_map, voxel_size=vs, epsilon=eps)
    if name == "mask":
        from sps_amd.baseline_filters import MaskFilter
        return MaskFilter(pc_map, voxel_size=vs)
    if name == "mos4d":
        from sps_amd.baseline_filters import MOS4DFilter
        from sps_amd.models.baselines import MOS4DNet
        if weights:
            return MOS4DFilter.from_checkpoint(weights)
        torch.manual_seed(0)
        return MOS4DFilter(MOS4DNet(0.2).cuda().eval().freeze(), buffer_size=10)
    if name == "mapmos":
        from sps_amd.baseline_filters import MapMOSFilter
        from sps_amd.models.baselines import MapMOSNet
        if weights:
            return MapMOSFilter.from_checkpoint(weights, pc_map[:, :3])
        torch.manual_seed(0)
        return MapMOSFilter(MapMOSNet(0.1).cuda().eval().freeze(), pc_map[:, :3])
    from sps_amd.lts_filter import LTSFilter
    from sps_amd.models.lts import SPCTReg
    torch.manual_seed(0)
    model = SPCTReg()
    if weights:
        model.load_state_dict(torch.load(weights, map_location="cpu", weights_only=False))
    return LTSFilter(model.cuda().eval(), lidar="hdl-32", epsilon_1=epsilon)


def frame_lines(name, res):
    """(the node's log lines of a frame, the numbers that enter the sequence means)."""
    if name in ("sps", "sps_cvm", "raw"):
        vals = {"T": res.t_total, "P": res.t_prune, "I": res.t_infer, "N": len(res.scores), "n": len(res.filtered)}
        if res.loss is not None:
            vals.update(loss=res.loss, r2=res.r2, dIoU=res.dIoU, accuracy=res.accuracy, precision=res.precision,
                        recall=res.recall, f1=res.f1)
        return list(res.log_lines()), vals
    if name == "mask":
        hz = lambda t: 1 / t if t else 0
        line = (f"T: {res.t_total:.3f} [{hz(res.t_total):.2f} Hz] P: {res.t_prune:.3f} [{hz(res.t_prune):.2f} Hz] "
                f"n: {len(res.filtered):d} S: {res.n_scan_voxels:d} M: {res.n_submap_voxels:d} ")
        return ["mask", line], {"T": res.t_total, "P": res.t_prune, "n": len(res.filtered)}
    vals = {"T": res.t_total, "I": res.t_infer, "n": len(res.filtered)}
    metrics = "no labels"
    if getattr(res, "dIoU", None) is not None:
        f1 = res.F1
        vals.update(dIoU=res.dIoU, accuracy=res.accuracy, precision=res.precision, recall=res.recall, f1=f1)
        metrics = (f"dIoU: {res.dIoU:.3f} accuracy: {res.accuracy:.3f} precision: {res.precision:.3f} "
                   f"recall: {res.recall:.3f} f1: {f1:.3f} ")
    return [metrics, f"T: {res.t_total:.3f} I: {res.t_infer:.3f} n: {len(res.filtered):d} "], vals


def submit(name, f, scan, T, prev_pose):
    if name == "sps_cvm":
        if prev_pose is not None:
            f.add_pose(prev_pose)                       # the corrected pose of the frame before: all the node ever has
        return f.submit(scan)
    if name == "lts":
        return f.submit(torch.from_numpy(np.ascontiguousarray(scan[:, :4], dtype=np.float32)).cuda())
    return f.submit(scan, T)


def hypothesis_grid(counts, steps, option="--hypotheses", step_option="--hypothesis-step", limit=64, what="hypotheses"):
    """--hypotheses NA,NB,NYAW / --hypothesis-step DA,DB,DYAW_DEG -> offsets [K, 4, 4]: a grid symmetric around 0 (odd
    counts) along, across and in yaw, with the identity moved to index 0.  --search / --search-step build theirs the same
    way, up to 65536 poses."""
    from sps_amd.localiser import pose_grid
    try:
        n = [int(v) for v in counts.split(",")]
        d = [float(v) for v in steps.split(",")]
    except ValueError:
        raise click.UsageError(f"{option} takes three integers, {step_option} three numbers")
    if len(n) != 3 or len(d) != 3 or any(v < 1 or v % 2 == 0 for v in n):
        raise click.UsageError(f"{option} takes three odd counts >= 1 (NA,NB,NYAW), {step_option} three steps")
    if n[0] * n[1] * n[2] > limit:
        raise click.UsageError(f"{option}: at most {limit} {what} in all")
    g = pose_grid(*[[(i - c // 2) * step for i in range(c)] for c, step in zip(n, d)])
    centre = ((n[0] // 2) * n[1] + n[1] // 2) * n[2] + n[2] // 2
    return np.concatenate([g[[centre]], np.delete(g, centre, axis=0)])


def closed_loop(name, f, pc_map, replay, finish, traj_out, which="icp", hypotheses=None, search=None, update_map=False,
                cell_capacity=None, max_cell_points=0, resolutions=None, level_iterations=None, carve_map=False,
                carve_options=None, level_capacities=None, estimator=None, source=None, coarse_to_fine=False,
                global_start=None, match_status=None, recover=None, inject=None, d2d=False, d2d_pyramid=False):
    """--localise: one LocalisationLoop step per frame, scored against the replayed poses.  ``estimator``: None, or the
    options of --estimator ukf (initial_velocity, scan_period, imu: None / a rate in Hz / an array of rows t ax .. gz).
    ``source``: None, or the keywords of NDTLocaliser(source="cells", ...) of --source cells.  ``coarse_to_fine``: hypotheses,
    search and the estimator's device path register on the pyramid of --resolutions.  ``d2d``: with ``source``, they
    register the scan's cells (--d2d); ``d2d_pyramid``: with ``source`` and its ``source_resolutions``, they register the
    scan's cells coarse to fine on the pyramid (--d2d-pyramid).  ``global_start``: None, or the
    options of --global-start (grid: the localiser's global_grid; yaw_steps, frontier, scan_z: of localise_global): the
    loop's initial pose is then found on the map from the first raw scan, and the sequence's first pose only scores it.
    ``match_status``: None, or the localiser's match_status of --match-status: every frame's inlier fraction and matching
    error are printed, and the lost and recovered frames counted at the end.  ``recover``: None, or the options of
    --recover-global (grid, and the loop's ``recover``).  ``inject``: None, or (frame, P) of --inject-jump: from that frame on
    the sensor stands at ``T @ P`` instead of T, so its scans are the replayed ones moved by the inverse of P, and the
    frames are scored against ``T @ P``."""
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser, ScanToMapLocaliser
    from sps_amd.trajectory import ape_translation, rotation_angle, write_trajectory
    skw = source or {}
    grid = global_start["grid"] if global_start is not None else recover["grid"] if recover is not None else None
    gkw = dict(global_grid=grid) if grid is not None else {}
    mkw = dict(match_status=match_status) if match_status is not None else {}
    lkw = dict(recover=recover["loop"]) if recover is not None else {}
    n_lost = n_recovered = 0
    if resolutions is not None and (update_map or carve_map):    # an online pyramid: per level, room for twice its cells
        caps = level_iterations or (30,) * len(resolutions)
        if level_capacities is None:
            xyz = np.ascontiguousarray(pc_map[:, :3], dtype=np.float64)
            level_capacities = tuple(max(2 * len(np.unique(np.floor(xyz / r).astype(np.int64), axis=0)), 4096) for r in resolutions)
        localiser = NDTLocaliser(pc_map[:, :3], resolutions=resolutions, iterations=sum(caps), level_iterations=caps,
                                 level_capacities=level_capacities, **skw, **gkw, **mkw)
    elif update_map or carve_map:                                # an online map: room for twice the map's cells by default
        n_cells = NDTLocaliser(pc_map[:, :3]).n_cells
        localiser = NDTLocaliser(pc_map[:, :3], cell_capacity=cell_capacity or max(2 * n_cells, 4096), **skw, **gkw, **mkw)
    elif resolutions is not None:                                # coarse to fine; hypotheses and search keep the single map
                                                                 # unless --coarse-to-fine sends them to the pyramid too
        caps = level_iterations or (30,) * len(resolutions)       # the budget is their sum: it cuts no level short
        localiser = NDTLocaliser(pc_map[:, :3], resolutions=resolutions, iterations=sum(caps), level_iterations=caps, **skw, **gkw,
                                 **mkw)
    else:
        localiser = NDTLocaliser(pc_map[:, :3], **skw, **gkw, **mkw) if which == "ndt" else ScanToMapLocaliser(pc_map[:, :3], **mkw)
    loop, stamps, ref, estimates = None, [], [], []
    for stamp, scan, pose, map_tr in replay:
        T = map_tr @ pose
        if inject is not None and len(stamps) >= inject[0]:
            Pi = np.linalg.inv(inject[1])
            scan = np.array(scan, copy=True)
            scan[:, :3] = (scan[:, :3].astype(np.float64) @ Pi[:3, :3].T + Pi[:3, 3]).astype(scan.dtype)
            T = T @ inject[1]
        if loop is None:
            est, T0 = None, T
            if global_start is not None:
                T0 = global_pose(localiser, scan, stamp, T, global_start, rotation_angle)
            if estimator is not None:
                from sps_amd.pose_estimator import PoseEstimator
                est = PoseEstimator(T0, localiser.device, initial_velocity=estimator["initial_velocity"])
            loop = LocalisationLoop(f, localiser, T0, hypotheses=hypotheses, search=search, update_map=update_map,
                                    max_cell_points=max_cell_points, carve_map=carve_map, carve_options=carve_options,
                                    estimator=est, coarse_to_fine=coarse_to_fine, **(dict(d2d=True) if d2d else {}),
                                    **(dict(d2d_pyramid=True) if d2d_pyramid else {}), **lkw)
            if est is not None:
                print("estimator: ukf  start of the registration: " + ("device pose" if loop.device_guess else "host pose"))
        if estimator is None:
            step = loop.step(scan)
        else:
            step = loop.step(scan, **frame_motion(estimator, len(stamps)))
            estimates.append(step.estimate)
        finish(stamp, None, step.filter_result)
        p = step.pose_result
        err_t = float(np.linalg.norm(step.pose[:3, 3] - T[:3, 3]))
        err_r = float(np.degrees(rotation_angle(step.pose, T)))
        print(f"[{stamp}] loc: {p.status:d} {p.iterations:d} {p.n_corr:d} {p.rmse:.4f} | {err_t:.4f} {err_r:.4f}"
              + (f" | {p.n_sources:d} sources" if source else "") + (" (flagged: the guess is kept)" if step.flagged else ""))
        if step.match is not None:
            m = step.match
            n_lost, n_recovered = n_lost + bool(m.lost), n_recovered + bool(step.recovered)
            print(f"[{stamp}] match: {m.inlier_fraction:.4f} {m.matching_error:.5f} | {m.n_inliers:d} of {m.n_valid:d} points"
                  + (" (lost)" if m.lost else "") + (" (recovered by the global search)" if step.recovered else ""))
        if p.levels is not None:
            print(f"[{stamp}] levels: slots per level " + " ".join(str(int((p.levels == l).sum())) for l in range(len(resolutions))))
        u = step.batch.map_update if step.batch is not None else p.map_update
        for l, ul in enumerate(u if isinstance(u, tuple) else () if u is None else (u,)):   # an online pyramid: one per level
            tag = f"map level {l}" if isinstance(u, tuple) else "map"
            print(f"[{stamp}] {tag}: {ul.cells:d} cells | founded {ul.founded:d} dropped {ul.dropped:d} | {ul.points:d} of "
                  f"{ul.n_points:d} points integrated")
        c = step.batch.map_carve if step.batch is not None else p.map_carve
        for l, cl in enumerate(c if isinstance(c, tuple) else () if c is None else (c,)):
            tag = f"carve level {l}" if isinstance(c, tuple) else "carve"
            print(f"[{stamp}] {tag}: {cl.rays:d} rays | seen through {cl.seen_through:d} cleared {cl.cleared:d} | cut {cl.cut:d}")
        if step.search is not None:
            r = step.search
            print(f"[{stamp}] search: pose {r.index:d} of {len(r.scores):d} | candidates " + " ".join(str(int(k)) for k in r.candidates)
                  + " | grid scores " + " ".join(f"{r.scores[k]:.1f}" for k in r.candidates if k >= 0))
        if step.batch is not None:
            b = step.batch
            print(f"[{stamp}] hypotheses: best {b.best:d} of {len(b.results):d} | scores "
                  + " ".join(f"{v:.1f}" for v in b.scores) + " | status " + " ".join(str(r.status) for r in b.results))
        stamps.append(stamp)
        ref.append(T)
    if loop is not None and stamps:
        ape = ape_translation(loop.poses, ref)
        print(f"APE translation (m) over {len(stamps)} frames: " + " ".join(f"{k}: {v:.4f}" for k, v in ape.items()))
        if estimates:
            ape = ape_translation(estimates, ref)
            print(f"APE translation (m) of the estimator over {len(stamps)} frames: " + " ".join(f"{k}: {v:.4f}" for k, v in ape.items()))
    if match_status is not None and stamps:
        print(f"scan matching over {len(stamps)} frames: lost {n_lost:d} recovered {n_recovered:d}")
    if traj_out:
        write_trajectory(traj_out, stamps, loop.poses if loop is not None else [])


def global_pose(localiser, scan, stamp, T, opts, rotation_angle):
    """--global-start: the initial pose of the loop from the first raw scan alone (NDTLocaliser.localise_global): the
    selected leaf, the certificate and the error against the sequence's first pose ``T`` are printed"""
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(scan)[:, :3], dtype=np.float32)).to(localiser.device)
    g = localiser.localise_global(rows, len(rows), opts["yaw_steps"], frontier=opts["frontier"], scan_z=opts["scan_z"]).result()
    s, grid = g.search, localiser._global
    print(f"[{stamp}] global: {s.n_slice:d} of {s.n_points:d} points in the slice | grid {grid['W']:d} x {grid['H']:d} | "
          f"candidates " + " ".join(str(int(v)) for v in s.candidates[::-1]) + " | kept " + " ".join(str(int(v)) for v in s.kept[::-1]))
    print(f"[{stamp}] global: certified {s.certified:d} of {s.n_found:d} | dropped {s.n_dropped:d}, bound {s.dropped_bound:d} | "
          f"scores " + " ".join(str(int(v)) for v in s.score[:s.n_found]))
    if not s.n_found:
        print(f"[{stamp}] global: no leaf found: the sequence's first pose starts the loop")
        return T
    k = g.batch.best if g.ok else 0
    a, j, i = s.leaf(k, grid["W"], grid["H"])
    T0 = g.pose if g.ok else s.poses[0]
    err_t = float(np.linalg.norm(T0[:3, 3] - T[:3, 3]))
    err_r = float(np.degrees(rotation_angle(T0, T)))
    leaf_t = float(np.linalg.norm(s.poses[k][:2, 3] - T[:2, 3]))
    print(f"[{stamp}] global: leaf {int(s.index[k]):d} (result {k:d}: yaw step {a:d} of {opts['yaw_steps']:d}, cell {i:d} {j:d}, "
          f"score {int(s.score[k]):d}, {leaf_t:.4f} m from the sequence's first pose)"
          + ("" if g.ok else " | no alignment was selected: the best leaf starts the loop"))
    print(f"[{stamp}] global: start pose | {err_t:.4f} {err_r:.4f}")
    return T0


def frame_motion(estimator, k):
    """the keywords of LocalisationLoop.step for frame k: the IMU rows of the interval that ends at scan k (scan k is at
    k * scan_period), or the interval alone"""
    S, imu = estimator["scan_period"], estimator["imu"]
    if imu is None or k == 0:
        return dict(dt=S)
    if np.ndim(imu) == 0:                                         # a rate: the synthetic sequence's own rows (it moves straight)
        from sps_amd import synthetic
        return dict(imu=synthetic.sequence_imu(2, scan_period=S, rate=float(imu))[1])
    rows = imu[(imu[:, 0] > (k - 1) * S) & (imu[:, 0] <= k * S)]
    if not len(rows):
        return dict(dt=S)
    out = rows.copy()
    out[:, 0] = np.diff(np.concatenate([[(k - 1) * S], rows[:, 0]]))
    return dict(imu=out)


@click.command()
@click.option("--filter", "name", type=click.Choice(FILTERS), default="sps")
@click.option("--weights", "-w", type=str, default=None, help="checkpoint of the chosen filter's model")
@click.option("--sequence", "-seq", type=str, default=None, help="sequence id under $DATA/sequence")
@click.option("--config", "-c", type=str, default=DEFAULT_CONFIG_PATH, help="Path to the config file (.yaml)")
@click.option("--epsilon", type=float, default=None, help="stability threshold (default: FILTER.THRESHOLD of the config)")
@click.option("--out", "out_dir", type=str, default=None, help="write the filtered clouds as DIR/<stamp>.npy")
@click.option("--synthetic", "n_synth", type=int, default=0, help="replay N synthetic scans instead of $DATA")
@click.option("--localise", is_flag=True, help="close the loop: localise every filtered cloud and feed the pose back")
@click.option("--localiser", "which", type=click.Choice(("icp", "ndt")), default=None,
              help="with --localise: point-to-point ICP (default) or NDT")
@click.option("--traj-out", "traj_out", type=str, default=None, help="with --localise: write the estimated trajectory")
@click.option("--hypotheses", "hyp_counts", type=str, default=None,
              help="with --localiser ndt: NA,NB,NYAW start poses (odd counts) along, across and in yaw around the guess")
@click.option("--hypothesis-step", "hyp_steps", type=str, default="0.5,0.5,5",
              help="with --hypotheses: DA,DB,DYAW_DEG, the grid's spacing in m, m and degrees")
@click.option("--search", "search_counts", type=str, default=None,
              help="with --localiser ndt: NA,NB,NYAW poses (odd counts) scored around the guess at the first frame and after "
                   "every flagged frame; the best 8 are registered")
@click.option("--search-step", "search_steps", type=str, default="1,0.5,5",
              help="with --search: DA,DB,DYAW_DEG, the grid's spacing in m, m and degrees")
@click.option("--update-map", "update_map", is_flag=True,
              help="with --localiser ndt: fold every frame's kept points into the NDT map at its corrected pose")
@click.option("--cell-capacity", "cell_capacity", type=int, default=None,
              help="with --update-map or --carve-map: cells the online map has room for (default: twice the map's, at least 4096)")
@click.option("--max-cell-points", "max_cell_points", type=int, default=0,
              help="with --update-map: cap on the weight of a cell's history (0: none)")
@click.option("--carve-map", "carve_map", is_flag=True,
              help="with --localiser ndt: cast every frame's kept points as rays from its corrected pose and clear the cells "
                   "of the NDT map that they keep passing through")
@click.option("--carve-miss-frames", "carve_miss_frames", type=int, default=None,
              help="with --carve-map: consecutive frames a cell must be seen through before it is cleared (default: 3)")
@click.option("--carve-sigma", "carve_sigma", type=float, default=None,
              help="with --carve-map: a ray passes through a cell within this many standard deviations of its mean (default: 1)")
@click.option("--resolutions", "resolutions", type=str, default=None,
              help="with --localiser ndt: R0,R1,... cell edges in m, strictly decreasing (at most 4): register coarse to fine")
@click.option("--level-iterations", "level_iterations", type=str, default=None,
              help="with --resolutions: N0,N1,... the most iterations each level may use (default: 30 each); their sum is the "
                   "frame's budget")
@click.option("--coarse-to-fine", "coarse_to_fine", is_flag=True,
              help="with --resolutions and one of --hypotheses, --search, --estimator ukf: these register on the pyramid too, "
                   "from start poses on the device (default: on the single 1 m map beside it)")
@click.option("--level-capacities", "level_capacities", type=str, default=None,
              help="with --resolutions and --update-map or --carve-map: C0,C1,... cells every level of the online pyramid has "
                   "room for (default per level: twice its cells, at least 4096)")
@click.option("--source", "source", type=click.Choice(("points", "cells")), default=None,
              help="with --localiser ndt: register the scan's points (default) or, distribution to distribution, one Gaussian "
                   "per cell of the scan; the loc: line then ends with the scan's valid source cells")
@click.option("--d2d", "d2d", is_flag=True,
              help="with --source cells and one of --hypotheses, --search, --estimator ukf: these register the scan's cells "
                   "too, distribution to distribution, from start poses on the device (without it --source cells takes "
                   "neither --hypotheses nor --search, and the estimator's guess is fetched to the host)")
@click.option("--d2d-pyramid", "d2d_pyramid", is_flag=True,
              help="with --source cells --resolutions --source-resolutions and one of --hypotheses, --search, --estimator ukf: "
                   "these register the scan's cells coarse to fine on the pyramid too, from start poses on the device")
@click.option("--source-resolution", "source_resolution", type=float, default=None,
              help="with --source cells: edge of the scan's cells in m (default: the map's resolution)")
@click.option("--source-min-points", "source_min_points", type=str, default=None,
              help="with --source cells: points a cell of the scan needs to be used (default: the map's); with "
                   "--source-resolutions also N0,N1,..., one per level")
@click.option("--source-resolutions", "source_resolutions", type=str, default=None,
              help="with --source cells --resolutions R0,R1,...: S0,S1,... the edge of the scan's cells at every level; the "
                   "scan's cells are then registered coarse to fine against the pyramid (without it --source cells takes "
                   "no --resolutions)")
@click.option("--global-start", "global_start", is_flag=True,
              help="with --localiser ndt: the loop's initial pose comes from a global search of the first raw scan on an "
                   "occupancy grid of the map (branch and bound over x, y, yaw), not from the sequence")
@click.option("--global-resolution", "global_resolution", type=float, default=0.5, help="with --global-start: cell edge in m")
@click.option("--global-map-z", "global_map_z", type=str, default="-1,3",
              help="with --global-start: LO,HI, the height slice of the map that makes the grid (map frame, m)")
@click.option("--global-scan-z", "global_scan_z", type=str, default="-1,3",
              help="with --global-start: LO,HI, the height slice of the scan that is matched (sensor frame, m)")
@click.option("--global-yaw-steps", "global_yaw_steps", type=int, default=72, help="with --global-start: headings tried")
@click.option("--global-levels", "global_levels", type=int, default=3, help="with --global-start: pooled levels of the grid")
@click.option("--global-frontier", "global_frontier", type=int, default=16384,
              help="with --global-start: nodes kept per level of the search")
@click.option("--match-status", "match_status", type=str, default=None, is_flag=False, flag_value="0.5",
              help="with --localise: DIST[,RANGE] (default 0.5): every registration is followed by the scan-matching status at "
                   "its pose -- the share of the thinned points within RANGE m of the sensor (default: all) that have a map "
                   "point within DIST m, and their mean squared distance -- printed per frame")
@click.option("--min-inlier-fraction", "min_inlier_fraction", type=float, default=0.0,
              help="with --match-status: a frame whose inlier fraction is below this is lost: flagged, the guess kept, the "
                   "online map and the estimator left alone")
@click.option("--recover-global", "recover_global", type=int, default=None,
              help="with --localiser ndt: after N flagged frames in a row the next frame is registered by the global search "
                   "(the --global-* options) instead of from the guess")
@click.option("--inject-jump", "inject_jump", type=str, default=None,
              help="with --localise: FRAME,DX,DY,YAW -- from that frame on the sensor is moved by (DX, DY) m and turned by YAW "
                   "degrees in its own frame against the replayed pose, unknown to the loop: a kidnap to test --match-status "
                   "and --recover-global with")
@click.option("--estimator", "estimator", type=click.Choice(("ukf",)), default=None,
              help="with --localise: the guess of every frame is the prediction of the device UKF pose estimator, which the "
                   "registered pose corrects; a second APE line is the estimator's")
@click.option("--initial-velocity", "initial_velocity", type=str, default="0,0,0",
              help="with --estimator: VX,VY,VZ in m/s, map frame (the filter learns a velocity slowly from zero)")
@click.option("--scan-period", "scan_period", type=float, default=0.1, help="with --estimator: seconds between scans")
@click.option("--imu-rate", "imu_rate", type=float, default=None,
              help="with --estimator and --synthetic: predict with the synthetic sequence's exact IMU rows at this rate in Hz")
@click.option("--imu", "imu_file", type=str, default=None,
              help="with --estimator: a text file of rows `t ax ay az gx gy gz`, scan k being at k * scan-period")
def main(name, weights, sequence, config, epsilon, out_dir, n_synth, localise, which, traj_out, hyp_counts, hyp_steps,
         search_counts, search_steps, update_map, cell_capacity, max_cell_points, carve_map, carve_miss_frames, carve_sigma,
         resolutions, level_iterations, coarse_to_fine, level_capacities, source, d2d, source_resolution, source_min_points, source_resolutions,
         estimator, initial_velocity, scan_period, imu_rate, imu_file, global_start, global_resolution, global_map_z,
         global_scan_z, global_yaw_steps, global_levels, global_frontier, match_status, min_inlier_fraction, recover_global,
         inject_jump, d2d_pyramid):
    if global_start and (which != "ndt" or not localise):
        raise click.UsageError("--global-start needs --localise --localiser ndt")
    if global_start and source == "cells":
        raise click.UsageError("--global-start takes no --source cells: the search matches points")
    if match_status is not None:
        if not localise:
            raise click.UsageError("--match-status needs --localise")
        try:
            v = [float(x) for x in match_status.split(",")]
        except ValueError:
            v = []
        if not 1 <= len(v) <= 2:
            raise click.UsageError("--match-status takes DIST[,RANGE]")
        match_status = dict(max_distance=v[0], min_inlier_fraction=min_inlier_fraction, **(dict(max_range=v[1]) if len(v) == 2 else {}))
    elif min_inlier_fraction:
        raise click.UsageError("--min-inlier-fraction needs --match-status")
    if recover_global is not None and (which != "ndt" or not localise or source == "cells" or recover_global < 1):
        raise click.UsageError("--recover-global needs N >= 1 and --localise --localiser ndt without --source cells")
    want_recover = recover_global is not None
    inject = None
    if inject_jump is not None:
        if not localise:
            raise click.UsageError("--inject-jump needs --localise")
        try:
            k, dx, dy, yaw = (float(x) for x in inject_jump.split(","))
        except ValueError:
            raise click.UsageError("--inject-jump takes FRAME,DX,DY,YAW")
        c, sn = math.cos(math.radians(yaw)), math.sin(math.radians(yaw))
        inject = (int(k), np.array([[c, -sn, 0.0, dx], [sn, c, 0.0, dy], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]))
    if global_start or want_recover:
        try:
            slices = [tuple(float(v) for v in z.split(",")) for z in (global_map_z, global_scan_z)]
        except ValueError:
            slices = [()]
        if any(len(z) != 2 for z in slices):
            raise click.UsageError("--global-map-z and --global-scan-z take LO,HI")
        global_opts = dict(grid=dict(resolution=global_resolution, map_z=slices[0], levels=global_levels), scan_z=slices[1],
                           yaw_steps=global_yaw_steps, frontier=global_frontier)
        global_start = global_opts if global_start else None
        recover_global = dict(grid=global_opts["grid"], loop=dict(after=recover_global, yaw_steps=global_yaw_steps,
                                                                  frontier=global_frontier, scan_z=slices[1])) if want_recover else None
    else:
        global_start = None
    if coarse_to_fine and (resolutions is None or (hyp_counts is None and search_counts is None and estimator is None)):
        raise click.UsageError("--coarse-to-fine needs --resolutions and one of --hypotheses, --search, --estimator ukf")
    if source is not None and (which != "ndt" or not localise):
        raise click.UsageError("--source needs --localise --localiser ndt")
    if (source_resolution is not None or source_min_points is not None) and source != "cells":
        raise click.UsageError("--source-resolution and --source-min-points need --source cells")
    if d2d and (source != "cells" or (hyp_counts is None and search_counts is None and estimator is None)):
        raise click.UsageError("--d2d needs --source cells and one of --hypotheses, --search, --estimator ukf")
    if source_resolutions is not None and (source != "cells" or resolutions is None or source_resolution is not None):
        raise click.UsageError("--source-resolutions needs --source cells and --resolutions, and no --source-resolution")
    if d2d_pyramid and (source != "cells" or resolutions is None or source_resolutions is None or d2d or coarse_to_fine
                        or (hyp_counts is None and search_counts is None and estimator is None)):
        raise click.UsageError("--d2d-pyramid needs --source cells, --resolutions, --source-resolutions and one of --hypotheses, "
                               "--search, --estimator ukf, and neither --d2d nor --coarse-to-fine")
    if source == "cells" and ((resolutions is not None and source_resolutions is None)
                              or ((hyp_counts is not None or search_counts is not None) and not (d2d or d2d_pyramid))):
        raise click.UsageError("--source cells takes no --resolutions, --hypotheses or --search: they register points"
                               " (--d2d lets --hypotheses and --search register the scan's cells; --source-resolutions "
                               "registers them on the pyramid of --resolutions)")
    try:
        if source_min_points is not None:
            mps = tuple(int(v) for v in source_min_points.split(","))
            source_min_points = mps[0] if len(mps) == 1 else mps
        if source_resolutions is not None:
            source_resolutions = tuple(float(v) for v in source_resolutions.split(","))
    except ValueError:
        raise click.UsageError("--source-min-points takes integers and --source-resolutions numbers, separated by commas")
    if isinstance(source_min_points, tuple) and source_resolutions is None:
        raise click.UsageError("a --source-min-points list needs --source-resolutions")
    if source == "cells":
        source = dict(source="cells", source_resolution=source_resolution, source_min_points=source_min_points)
        if source_resolutions is not None:
            source["source_resolutions"] = source_resolutions
    else:
        source = None
    if estimator is None and (initial_velocity != "0,0,0" or imu_rate is not None or imu_file is not None):
        raise click.UsageError("--initial-velocity, --imu-rate and --imu need --estimator")
    if estimator is not None:
        if not localise:
            raise click.UsageError("--estimator needs --localise")
        if imu_rate is not None and imu_file is not None:
            raise click.UsageError("give --imu-rate or --imu, not both")
        if imu_rate is not None and not n_synth:
            raise click.UsageError("--imu-rate makes the synthetic sequence's IMU rows: it needs --synthetic")
        try:
            vel = tuple(float(v) for v in initial_velocity.split(","))
        except ValueError:
            vel = ()
        if len(vel) != 3 or not scan_period > 0 or (imu_rate is not None and not imu_rate > 0):
            raise click.UsageError("--initial-velocity takes VX,VY,VZ; --scan-period and --imu-rate must be > 0")
        imu = imu_rate
        if imu_file is not None:
            imu = np.loadtxt(imu_file, dtype=np.float64, ndmin=2)
            if imu.shape[1] != 7 or not np.isfinite(imu).all() or (np.diff(imu[:, 0]) <= 0).any():
                raise click.UsageError("--imu: rows `t ax ay az gx gy gz`, finite, t strictly increasing")
        estimator = dict(initial_velocity=vel, scan_period=float(scan_period), imu=imu)
    if carve_map and which != "ndt":
        raise click.UsageError("--carve-map needs --localise --localiser ndt")
    if (carve_miss_frames is not None or carve_sigma is not None) and not carve_map:
        raise click.UsageError("--carve-miss-frames and --carve-sigma need --carve-map")
    carve_options = {}
    if carve_miss_frames is not None:
        carve_options["miss_frames"] = carve_miss_frames
    if carve_sigma is not None:
        carve_options["through_sigma"] = carve_sigma
    if resolutions is not None and which != "ndt":
        raise click.UsageError("--resolutions needs --localise --localiser ndt")
    if level_iterations is not None and resolutions is None:
        raise click.UsageError("--level-iterations needs --resolutions")
    if level_capacities is not None and resolutions is None:
        raise click.UsageError("--level-capacities needs --resolutions")
    if level_capacities is not None and not (update_map or carve_map):
        raise click.UsageError("--level-capacities needs --update-map or --carve-map")
    try:
        resolutions = None if resolutions is None else tuple(float(v) for v in resolutions.split(","))
        level_iterations = None if level_iterations is None else tuple(int(v) for v in level_iterations.split(","))
        level_capacities = None if level_capacities is None else tuple(int(v) for v in level_capacities.split(","))
    except ValueError:
        raise click.UsageError("--resolutions takes numbers, --level-iterations and --level-capacities integers, separated by commas")
    if resolutions is not None and (update_map or carve_map):
        if cell_capacity is not None:
            raise click.UsageError("--cell-capacity is the single map's: with --resolutions give --level-capacities")
        if (hyp_counts is not None or search_counts is not None) and not (coarse_to_fine or d2d_pyramid):
            raise click.UsageError("--resolutions with --update-map or --carve-map takes no --hypotheses and no --search: they "
                                   "register on the single map, which stays static")
        if recover_global is not None and not coarse_to_fine:
            raise click.UsageError("--resolutions with --update-map or --carve-map takes no --recover-global without "
                                   "--coarse-to-fine: the global search registers on the single map, which stays static")
    if update_map and which != "ndt":
        raise click.UsageError("--update-map needs --localise --localiser ndt")
    if max_cell_points and not update_map:
        raise click.UsageError("--max-cell-points needs --update-map")
    if cell_capacity is not None and not (update_map or carve_map):
        raise click.UsageError("--cell-capacity needs --update-map or --carve-map")
    if which is not None and not localise:
        raise click.UsageError("--localiser needs --localise")
    if hyp_counts is not None and which != "ndt":
        raise click.UsageError("--hypotheses needs --localise --localiser ndt")
    if search_counts is not None and which != "ndt":
        raise click.UsageError("--search needs --localise --localiser ndt")
    hypotheses = hypothesis_grid(hyp_counts, hyp_steps) if hyp_counts is not None else None
    search = hypothesis_grid(search_counts, search_steps, "--search", "--search-step", 65536, "poses") \
        if search_counts is not None else None
    cfg = yaml.safe_load(open(config))
    if epsilon is None:
        epsilon = float(cfg.get("FILTER", {}).get("THRESHOLD", 0.84))
    tmp = None
    if n_synth:
        tmp = tempfile.TemporaryDirectory()
        data_dir, sequence = tmp.name, "synthetic"
        write_synthetic_tree(data_dir, n_synth, sequence)
    else:
        assert sequence, "give -seq SEQ or --synthetic N"
        data_dir = str(os.environ.get("DATA"))
    replay = ScanReplay(data_dir, sequence)
    map_pth = os.path.join(data_dir, "maps", cfg["TRAIN"]["MAP"] if not n_synth else "base_map.asc.npy")
    pc_map = np.load(map_pth) if map_pth.endswith(".npy") else np.loadtxt(map_pth, dtype=np.float32)
    f = build_filter(name, cfg, weights, torch.from_numpy(np.ascontiguousarray(pc_map[:, :3], dtype=np.float32)), epsilon)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    print(f"filter: {name}  sequence: {sequence}  scans: {len(replay)}  epsilon: {RAW_EPSILON if name == 'raw' else epsilon}")

    totals, n_done = {}, 0

    def finish(stamp, pend, res=None):
        nonlocal n_done
        res = pend.result() if res is None else res
        lines, vals = frame_lines(name, res)
        for line in lines:
            print(f"[{stamp}] {line}")
        for k, v in vals.items():
            totals.setdefault(k, []).append(float(v))
        if out_dir:
            np.save(os.path.join(out_dir, stamp + ".npy"), res.filtered.cpu().numpy())
        n_done += 1

    if localise:
        closed_loop(name, f, pc_map, replay, finish, traj_out, which or "icp", hypotheses, search, update_map, cell_capacity,
                    max_cell_points, resolutions, level_iterations, carve_map, carve_options or None, level_capacities,
                    estimator, source, coarse_to_fine, global_start, match_status, recover_global, inject, d2d, d2d_pyramid)
    elif traj_out:
        raise click.UsageError("--traj-out needs --localise")
    in_flight, prev_pose = None, None
    for stamp, scan, pose, map_tr in ([] if localise else replay):
        T = map_tr @ pose
        pend = submit(name, f, scan, T, prev_pose)
        prev_pose = T
        if in_flight is not None:
            finish(*in_flight)                          # frame i's result after frame i + 1's submit
        in_flight = (stamp, pend)
    if in_flight is not None:
        finish(*in_flight)
    means = " ".join(f"{k}: {np.mean(v):.3f}" for k, v in totals.items())
    print(f"sequence means over {n_done} frames: {means}")
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
