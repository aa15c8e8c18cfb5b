"""CPU tests of distribution-to-distribution NDT from several poses: the selection and top-K rules the
restatement (tests/ndt_d2d_batch_reference.py) composes, the scene the GPU test re-uses, the ``d2d=True`` checks that need
no device, the loop's routing, the header and the drivers' options.  No GPU."""
import functools
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from tests import localiser_reference as LR
from tests import ndt_batch_reference as NB
from tests import ndt_d2d_batch_reference as DBR
from tests import ndt_d2d_reference as DR
from tests import ndt_reference as NR
from tests import ndt_search_reference as NS
from tests.test_ndt_d2d_cpu import EIG_RATIO, KW, T_INIT, sensor_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 0.4
ALONG, ACROSS, YAW = (-1.5, 0.0, 1.5), (-1.0, 0.0, 1.0), (0.0, 8.0)          # the 18 start poses of tests/test_ndt_batch_cpu.py
CENTRE = (1 * len(ACROSS) + 1) * len(YAW) + 0
G_ALONG, G_ACROSS, G_YAW = (-1.0, -0.5, 0.0, 0.5, 1.0), (-0.5, 0.0, 0.5), (-4.0, 0.0, 4.0)   # the 45 poses of the scored grid
SYMBOLS = ("sps_ndt_align_d2d_batch_scratch", "sps_ndt_align_d2d_batch", "sps_ndt_score_d2d_scratch", "sps_ndt_score_poses_d2d")


@functools.lru_cache(maxsize=1)
def scene_d2d():
    """The scene of tests/test_hip_ndt_d2d.py at leaf 0.4 (246 valid source cells) registered by the restatement from 18
    start poses T_INIT @ D(a, b, psi), and scored on a grid of 45.  Computed once per process, shared with the GPU test,
    never modified."""
    from sps_amd import synthetic
    map_xyz = synthetic.build_map(**KW)[:, :3].astype(np.float64)
    cmap = NR.cells(map_xyz, 1.0)
    scan = sensor_scan(1)
    pts = LR.downsample(scan, len(scan), LEAF)[1]
    src = DR.sources(pts, 1.0, 6, EIG_RATIO)
    starts = np.stack([T_INIT @ d for d in NB.grid(ALONG, ACROSS, YAW)])
    grid = np.stack([T_INIT @ d for d in NB.grid(G_ALONG, G_ACROSS, G_YAW)])
    return dict(map_xyz=map_xyz, cmap=cmap, scan=scan, pts=pts, src=src, starts=starts, grid=grid,
                ref=DBR.align_batch(src, cmap, starts), rev=DR.align(src, cmap, starts[CENTRE], reverse=True),
                ref_grid=DBR.score_poses(src, cmap, grid))


# ---- the rules the restatement composes -------------------------------------------------------------------------------------
def test_select_on_hand_made_scores():
    sel = DBR.select
    assert sel([1.0, 3.0, 3.0], [100] * 3, [0, 1, 0], 50) == 1               # a tie goes to the lowest index
    assert sel([3.0, 3.0, 2.0], [100] * 3, [1, 0, 0], 50) == 0
    assert sel([math.nan, 2.0, math.nan], [100] * 3, [0, 0, 0], 50) == 1     # NaN never wins, wherever it stands
    assert sel([2.0, math.nan], [100] * 2, [0, 0], 50) == 0
    assert sel([math.nan, math.nan], [100] * 2, [0, 0], 50) == -1
    assert sel([1.0, 3.0, 2.0], [100] * 3, [0, 2, 1], 50) == 2               # status 2 and 3 are out whatever their score
    assert sel([1.0, 3.0, 2.0], [100, 49, 50], [0, 0, 0], 50) == 2           # sources counted below min_corr
    assert sel([1.0, 3.0], [100, 100], [2, 3], 50) == -1                     # nobody qualifies
    assert sel([], [], [], 50) == -1


def test_top_on_hand_made_scores():
    idx, n = NS.top([3.0, 1.0, 3.0, 3.0], [100] * 4, 50, 3)
    assert list(idx) == [0, 2, 3] and n == 3                                  # ties keep the lowest index first
    idx, n = NS.top([math.nan, 1.0, 2.0], [100] * 3, 50, 2)
    assert list(idx) == [2, 1] and n == 2                                     # NaN does not qualify
    idx, n = NS.top([5.0, 1.0, 2.0], [10, 100, 49], 50, 4)
    assert list(idx) == [1, -1, -1, -1] and n == 1                            # fewer than K qualify
    idx, n = NS.top([5.0, 1.0], [0, 0], 50, 2)
    assert list(idx) == [-1, -1] and n == 0                                   # nobody qualifies
    poses = np.arange(3 * 16, dtype=np.float64).reshape(3, 4, 4)
    assert NS.top_poses(poses, np.array([1, -1])).tobytes() == poses[[1, 1]].tobytes()   # an unfilled slot: the pose of slot 0
    assert NS.top_poses(poses, np.array([-1, -1])).tobytes() == poses[[0, 0]].tobytes()  # nobody: poses[0]


# ---- the scene of the GPU test ----------------------------------------------------------------------------------------------
def test_the_scene_needs_no_face_and_no_guard_boundary():
    s = scene_d2d()
    assert s["src"]["n_src"][1] == 246 and len(s["starts"]) == 18 and len(s["grid"]) == 45
    ref = s["ref"]
    for k, r in enumerate(ref["results"]):
        assert r["faces"] == 0 and r["boundary"] == 0, k
        assert ref["hits"][k]["faces"] == 0 and ref["hits"][k]["boundary"] == 0, k
    assert s["rev"]["faces"] == 0 and s["rev"]["boundary"] == 0
    assert (s["ref_grid"]["faces"] == 0).all() and (s["ref_grid"]["boundary"] == 0).all()
    courses = {(r["status"], r["iterations"]) for r in ref["results"]}
    print("courses of the 18 hypotheses:", sorted(courses), "best", ref["best"], "counts", list(ref["counts"]))
    assert len(courses) > 1                                                   # the hypotheses do not all take the same course
    assert ref["best"] >= 0 and ref["results"][CENTRE]["status"] == 0
    assert ref["pose"].tobytes() == ref["results"][ref["best"]]["pose"].tobytes()


def test_the_restatement_composes_and_adds_nothing():
    s = scene_d2d()
    src, cmap, ref = s["src"], s["cmap"], s["ref"]
    one = DR.align(src, cmap, s["starts"][3])
    assert ref["results"][3]["pose"].tobytes() == one["pose"].tobytes() and ref["results"][3]["trace"].tobytes() == one["trace"].tobytes()
    sc, h = DR.score(src, cmap, one["pose"])
    assert ref["scores"][3] == sc and ref["counts"][3] == len(np.unique(h["i"]))
    g = s["ref_grid"]
    zero = DBR.align_batch(src, cmap, s["grid"][:4], iters=0)                 # the zero-iteration batch is the score of the grid
    assert zero["scores"].tobytes() == g["scores"][:4].tobytes() and zero["counts"].tobytes() == g["counts"][:4].tobytes()
    assert [r["status"] for r in zero["results"]] == [1] * 4
    # the device's order of summation stays within the bound the GPU test uses against math.fsum
    assert (np.abs(g["ordered"] - g["scores"]) <= (g["m"] + 6) * 2.0 ** -52 * g["sum_abs"]).all()
    rel = DBR.relocalise(src, cmap, s["grid"], keep=4)
    idx, n = NS.top(g["scores"], g["counts"], 50, 4)
    assert list(rel["candidates"]) == list(idx) and rel["n_top"] == n == 4 and rel["index"] == idx[rel["batch"]["best"]]
    # a pose that is not finite, one off the map and an empty map score (0, 0)
    bad = s["grid"][:3].copy()
    bad[0, 0, 0], bad[1, 0, 3] = np.nan, 5000.0
    b = DBR.score_poses(src, cmap, bad)
    assert list(b["scores"][:2]) == [0.0, 0.0] and list(b["counts"]) == [0, 0, g["counts"][2]] and b["scores"][2] == g["scores"][2]
    e = DBR.score_poses(src, NR.cells(np.zeros((0, 3)), 1.0), s["grid"][:2])
    assert list(e["scores"]) == [0.0, 0.0] and list(e["counts"]) == [0, 0]
    none = DBR.align_batch(src, NR.cells(np.zeros((0, 3)), 1.0), s["starts"][:3])
    assert none["best"] == -1 and none["pose"].tobytes() == s["starts"][0].tobytes()


# ---- the checks of d2d=True that need no device -------------------------------------------------------------------------------
def bare(**kw):
    """an NDTLocaliser that was never opened: the checks in front of the device work are all it can do"""
    from sps_amd.localiser import NDTLocaliser
    loc = object.__new__(NDTLocaliser)
    for k, v in dict(dict(source="cells", resolutions=None, level_capacities=None, cell_capacity=None, resolution=1.0), **kw).items():
        setattr(loc, k, v)
    return loc


def test_d2d_refusals_come_before_any_device_work():
    T = np.eye(4)[None]
    calls = dict(submit_batch=lambda l, **kw: l.submit_batch(None, 0, T, **kw),
                 submit_from_device=lambda l, **kw: l.submit_from_device(None, 0, None, **kw),
                 score_poses=lambda l, **kw: l.score_poses(None, 0, T, **kw),
                 relocalise=lambda l, **kw: l.relocalise(None, 0, T, **kw))
    for name, call in calls.items():
        with pytest.raises(ValueError, match="d2d=True needs an NDTLocaliser with source='cells'"):
            call(bare(source="points"), d2d=True)
        with pytest.raises(ValueError, match="source='points'"):               # without the keyword: refused as ever
            call(bare())
        with pytest.raises(ValueError, match="source='points'"):
            call(bare(), d2d=False)
        if name != "score_poses":
            with pytest.raises(ValueError, match="d2d=True and coarse_to_fine exclude each other"):
                call(bare(), d2d=True, coarse_to_fine=True)
            with pytest.raises(ValueError, match="d2d=True and coarse_to_fine exclude each other"):
                call(bare(resolutions=(2.0, 1.0)), d2d=True, coarse_to_fine=True)
            with pytest.raises(ValueError, match="online map"):                # the map operations keep their checks
                call(bare(), d2d=True, integrate=True)
        with pytest.raises(TypeError, match="needs a tensor"):                  # accepted: the next check, of the rows, fails
            call(bare(), d2d=True)
    for name in ("submit_filtered_batch", "relocalise_filtered"):
        pend = type("Pending", (), dict(_filtered=None, count_dev=None))()
        with pytest.raises(ValueError, match="d2d=True needs"):
            getattr(bare(source="points"), name)(pend, T, d2d=True)
    for keep in (0, 65):
        with pytest.raises(ValueError, match="keep must be in"):
            bare().relocalise(None, 0, T, keep=keep, d2d=True)
    for bad in (np.full((2, 4, 4), np.nan), np.zeros((0, 4, 4)), np.eye(4), np.stack([np.eye(4), np.full((4, 4), np.inf)])):
        for name in ("submit_batch", "score_poses", "relocalise"):
            with pytest.raises(ValueError, match="must be finite"):
                getattr(bare(), name)(None, 0, bad, d2d=True)
    with pytest.raises(ValueError, match="1 <= K <= 64"):
        bare().submit_batch(None, 0, np.tile(np.eye(4), (65, 1, 1)), d2d=True)


def test_a_d2d_batch_buffer_parses_with_the_sources():
    from sps_amd.localiser import PendingPoses, _batch_layout
    K, I = 2, 3
    o = _batch_layout(K, I, False)
    h = np.zeros(o["total"])
    h[o["status"]:o["n_points"]].view(np.int32)[:] = [0, 2, 70, 0, 2, 1, 3, 0]
    h[o["n_points"]:o["best"]].view(np.int32)[:] = [4157, 246]
    h[o["best"]:o["T_best"]].view(np.int32)[:] = [0, 0, 70, K]
    r = PendingPoses(K, I, False, None, None, None)._parse(h)
    assert [(x.n_points, x.n_sources, x.n_corr) for x in r.results] == [(4157, 246, 70), (4157, 246, 3)]
    r = PendingPoses(K, I, False, None, None, None)._parse(np.zeros(o["total"]))   # a point batch leaves the pad zero
    assert [x.n_sources for x in r.results] == [0, 0]


# ---- the loop's routing ---------------------------------------------------------------------------------------------------------
class TakesNone:
    takes_pose = False


class TakesPose:
    pass


class Est:
    pose_dev = None

    def predict(self, dt): ...
    def predict_imu(self, s): ...
    def correct_from(self, p): ...
    def snapshot(self): ...


class Cells:
    source = "cells"
    device = "cpu"

    def submit_from_device(self, *a, **k): ...
    def submit_batch(self, *a, **k): ...
    def relocalise(self, *a, **k): ...


class Points(Cells):
    source = "points"


def test_the_loop_options():
    from sps_amd.localiser import LocalisationLoop
    eye, grid = np.eye(4), np.eye(4)[None]
    with pytest.raises(ValueError, match="d2d=True needs an NDTLocaliser with source='cells'"):
        LocalisationLoop(TakesNone(), Points(), eye, d2d=True)
    with pytest.raises(ValueError, match="d2d=True needs an NDTLocaliser with source='cells'"):
        LocalisationLoop(TakesNone(), object(), eye, d2d=True)
    with pytest.raises(ValueError, match="d2d=True and coarse_to_fine exclude each other"):
        LocalisationLoop(TakesNone(), Cells(), eye, d2d=True, coarse_to_fine=True)
    for kw in (dict(hypotheses=grid), dict(search=grid)):
        with pytest.raises(ValueError, match="source='points'"):               # without the argument: refused as ever
            LocalisationLoop(TakesNone(), Cells(), eye, **kw)
        with pytest.raises(ValueError, match="source='points'"):
            LocalisationLoop(TakesNone(), Cells(), eye, d2d=False, **kw)
        loop = LocalisationLoop(TakesNone(), Cells(), eye, d2d=True, **kw)
        assert loop.d2d is True and (loop.hypotheses is not None or loop.search is not None)
        assert LocalisationLoop(TakesNone(), Cells(), eye, d2d=True, estimator=Est(), **kw).device_guess is False
        with pytest.raises(ValueError, match="device_guess=True needs"):
            LocalisationLoop(TakesNone(), Cells(), eye, d2d=True, estimator=Est(), device_guess=True, **kw)
    # the device path: with d2d only, and under the same conditions on the filter as for points
    assert LocalisationLoop(TakesNone(), Cells(), eye, estimator=Est()).device_guess is False
    with pytest.raises(ValueError, match="device_guess=True needs"):
        LocalisationLoop(TakesNone(), Cells(), eye, estimator=Est(), device_guess=True)
    assert LocalisationLoop(TakesNone(), Cells(), eye, estimator=Est(), d2d=True).device_guess is True
    assert LocalisationLoop(TakesNone(), Cells(), eye, estimator=Est(), d2d=True, device_guess=True).device_guess is True
    assert LocalisationLoop(TakesNone(), Cells(), eye, estimator=Est(), d2d=True, device_guess=False).device_guess is False
    assert LocalisationLoop(TakesPose(), Cells(), eye, estimator=Est(), d2d=True).device_guess is False
    with pytest.raises(ValueError, match="device_guess=True needs"):
        LocalisationLoop(TakesPose(), Cells(), eye, estimator=Est(), d2d=True, device_guess=True)
    with pytest.raises(ValueError, match="device_guess needs an estimator"):
        LocalisationLoop(TakesNone(), Cells(), eye, d2d=True, device_guess=True)
    assert LocalisationLoop(TakesNone(), Points(), eye, estimator=Est()).device_guess is True   # points: as ever
    assert LocalisationLoop(TakesNone(), Points(), eye).d2d is False


class Recorder(Cells):
    """a cells localiser that records how the loop calls it and answers with one converged hypothesis"""

    def __init__(self):
        self.calls = []

    def _answer(self, name, args, kw):
        from sps_amd.localiser import BatchPoseResult, PoseResult, RelocalisationResult
        self.calls.append((name, kw))
        one = PoseResult(np.eye(4), 0, 1, 60, 0.0, np.zeros((1, 4)))
        batch = BatchPoseResult([one], np.zeros(1), np.zeros(1, np.int64), 0, np.eye(4))
        out = dict(submit=one, submit_batch=batch, submit_from_device=batch,
                   relocalise=RelocalisationResult(np.zeros(1), np.zeros(1, np.int64), np.zeros(1, np.int64), batch, 0, np.eye(4)))[name]
        return type("Done", (), dict(result=lambda self: out))()

    def submit(self, rows, count, *a, **kw):
        return self._answer("submit", a, kw)

    def submit_batch(self, rows, count, *a, **kw):
        return self._answer("submit_batch", a, kw)

    def relocalise(self, rows, count, *a, **kw):
        return self._answer("relocalise", a, kw)

    def submit_from_device(self, rows, count, *a, **kw):
        return self._answer("submit_from_device", a, kw)


class HostFilter:
    """takes no pose; its rows come with the result, so the loop registers behind it"""
    takes_pose = False

    def submit(self, scan):
        res = type("Result", (), dict(filtered=scan))()
        return type("Pending", (), dict(result=lambda self: res))()


class RecordingEst(Est):
    pose_dev = "the estimator's device pose"

    def __init__(self):
        self.corrected = []

    def correct_from(self, p):
        self.corrected.append(p)

    def snapshot(self):
        state = type("State", (), dict(pose=np.eye(4)))()
        return lambda: (state, np.eye(4))


def test_the_loop_passes_d2d_to_the_batch_the_search_and_the_device_path_and_nothing_else():
    import torch

    from sps_amd.localiser import LocalisationLoop
    scan, eye, grid = torch.zeros((3, 4)), np.eye(4), np.eye(4)[None]
    loc = Recorder()
    LocalisationLoop(HostFilter(), loc, eye, hypotheses=grid, d2d=True).step(scan)
    assert loc.calls == [("submit_batch", dict(d2d=True))]
    loc = Recorder()
    loop = LocalisationLoop(HostFilter(), loc, eye, search=grid, hypotheses=grid, search_keep=3, d2d=True)
    loop.step(scan), loop.step(scan)
    assert loc.calls == [("relocalise", dict(d2d=True, keep=3)), ("submit_batch", dict(d2d=True))]
    loc = Recorder()
    LocalisationLoop(HostFilter(), loc, eye, d2d=True).step(scan)             # the plain registration is D2D already
    assert loc.calls == [("submit", {})]
    loc, est = Recorder(), RecordingEst()
    loop = LocalisationLoop(HostFilter(), loc, eye, estimator=est, d2d=True)
    step = loop.step(scan)
    assert loop.device_guess is True and loc.calls == [("submit_from_device", dict(d2d=True))]
    assert len(est.corrected) == 1 and step.batch is not None and not step.flagged
    loc, est = Recorder(), RecordingEst()                                      # without d2d: the guess is fetched, submit it is
    est.pose_dev = torch.eye(4, dtype=torch.float64)
    loop = LocalisationLoop(HostFilter(), loc, eye, estimator=est)
    loop.step(scan)
    assert loop.device_guess is False and loc.calls == [("submit", {})]


# ---- the header, the binding, the drivers -------------------------------------------------------------------------------------------
def test_the_header_declares_the_four_symbols():
    text = open(os.path.join(ROOT, "include", "sps_hip.h")).read()
    assert "NDT localiser, distribution to distribution, several poses" in text
    for name in SYMBOLS:
        assert re.search(r"^int(64_t)? " + name + r"\(", text, re.M), name
    assert re.search(r"int sps_ndt_align_d2d_batch\(sps_ctx \*ctx, const double \*src_dev, const int32_t \*n_src_dev, int64_t cap_src,\s+"
                     r"const double \*T_init_dev, int n_hyp, int iters, int neighbours, int min_corr, double outlier_ratio,\s+"
                     r"double tol_t, double tol_r, double \*T_out_dev, int32_t \*status_dev, double \*trace_dev,\s+"
                     r"double \*normal_dev, double \*final_dev, int32_t \*best_dev, double \*T_best_dev, void \*scratch_dev,\s+"
                     r"void \*stream\);", text)


def test_the_binding_knows_the_entry_points():
    from sps_amd import _native
    for name in SYMBOLS:
        assert name in _native.EXPORTS and hasattr(_native.lib, name), name
    lib = _native.lib
    assert lib.sps_version() == _native.ABI_VERSION == 202                     # additive: the ABI version does not change
    assert lib.sps_ndt_align_d2d_batch_scratch(1000, 18) == lib.sps_ndt_align_batch_scratch(1000, 18) > 0
    assert lib.sps_ndt_score_d2d_scratch(1000, 4096) == lib.sps_ndt_score_scratch(1000, 4096) > 0
    for cap, k in ((-1, 1), (1 << 24, 1), (100, 0), (100, 65)):
        assert lib.sps_ndt_align_d2d_batch_scratch(cap, k) == -1
    for cap, p in ((-1, 1), (1 << 24, 1), (100, 0), (100, 65537)):
        assert lib.sps_ndt_score_d2d_scratch(cap, p) == -1
    # the chunks of the scorer: the scratch stays at or below 64 MiB until one tile of 32 poses alone needs more
    assert lib.sps_ndt_score_d2d_scratch(2048, 65536) == 65536 * 64 * 16 == 64 << 20
    assert lib.sps_ndt_score_d2d_scratch(2049, 65536) == 64512 * 65 * 16 <= 64 << 20


def test_the_driver_option():
    """through click's own runner, in this process: every case ends in the option checks, before any device work"""
    from click.testing import CliRunner
    spec = importlib.util.spec_from_file_location("filter_sequence_under_test", os.path.join(ROOT, "scripts", "filter_sequence.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)

    def run(*opts):
        return CliRunner().invoke(script.main, ["--synthetic", "2", "--localise", "--localiser", "ndt", *opts])
    r = CliRunner().invoke(script.main, ["--help"])
    assert r.exit_code == 0 and "--d2d" in r.output
    needs = "--d2d needs --source cells and one of --hypotheses, --search, --estimator ukf"
    for opts in (("--d2d",), ("--d2d", "--hypotheses", "3,1,1"), ("--d2d", "--source", "cells"),
                 ("--d2d", "--source", "points", "--estimator", "ukf")):
        r = run(*opts)
        assert r.exit_code == 2 and needs in r.output, opts
    for opts in (("--hypotheses", "3,1,1"), ("--search", "3,1,1")):             # without the flag: the message as ever
        r = run("--source", "cells", *opts)
        assert r.exit_code == 2 and "--source cells takes no --resolutions, --hypotheses or --search" in r.output, opts
    r = run("--source", "cells", "--d2d", "--hypotheses", "3,1,1", "--resolutions", "2,1")
    assert r.exit_code == 2 and "--source cells takes no --resolutions" in r.output
