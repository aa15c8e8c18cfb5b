"""CPU tests of the coarse-to-fine NDT batch: the inputs of tests/test_hip_ndt_pyramid_batch.py on the restatement
(tests/ndt_pyramid_batch_reference.py), the selection rule on hand-made tables, and the argument and option logic of
NDTLocaliser, LocalisationLoop and the driver with stand-in objects.  No GPU."""
import math
import os

import numpy as np
import pytest

from tests import localiser_reference as LR
from tests import ndt_pyramid_batch_reference as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ---- the inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [0, 1, 2])
def test_the_inputs_have_the_properties_the_gpu_tests_rely_on(budget):
    r = B.restated(budget)
    res = r["results"]
    for k, x in enumerate(res):
        print(f"{B.BUDGETS[budget]} {B.NAMES[k]:12s}: status {x['status']} slots {x['iterations']} first slot of each level "
              f"{B.entered(x['levels'])} error {LR.pose_difference(x['pose'], B.T_TRUE)[0]:.4f} m finest-level score "
              f"{r['scores'][k]:.4f} count {r['counts'][k]}")
        assert x["faces"] == 0 and x["boundary"] == 0                          # exact counts need such an input
    B.check_input_properties(budget, [x["status"] for x in res], [x["iterations"] for x in res], [x["levels"] for x in res],
                             [x["pose"] for x in res], r["scores"])
    # the selection: never the start off the map, never the wrong basin; with four slots one that never reached level 2
    assert r["best"] not in (B.OFF, B.WRONG) and r["best"] >= 0
    assert r["pose"].tobytes() == res[r["best"]]["pose"].tobytes()
    if budget == 0:
        assert r["scores"][r["best"]] > r["scores"][B.WRONG] + 100.0
    if budget == 2:
        assert 2 not in res[r["best"]]["levels"] and res[r["best"]]["status"] == 1
    assert r["scores"][B.OFF] == 0.0 and r["counts"][B.OFF] == 0


def test_a_batch_of_the_start_off_the_map_selects_nobody():
    sc = B.scene()
    r = B.align_batch(sc["pts"], sc["cmaps"], B.POSES[[B.OFF, B.OFF]], 4, (2, 2, 2))
    assert r["best"] == -1 and r["pose"].tobytes() == B.POSES[B.OFF].tobytes()
    assert B.best_words(r["best"], [x["status"] for x in r["results"]], r["counts"], 2) == [-1, -1, 0, 2]


# ---- the selection rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("statuses,counts,scores,want", [
    ((0, 0, 0), (60, 60, 60), (1.0, 3.0, 2.0), 1),
    ((0, 1, 0), (60, 60, 60), (2.0, 2.0, 2.0), 0),                             # a tie stays with the lowest index
    ((2, 1, 0), (60, 60, 60), (9.0, 2.0, 2.0), 1),                             # ... among those that qualify
    ((0, 1, 3), (60, 49, 60), (1.0, 9.0, 9.0), 0),                             # too few points counted; status 3
    ((0, 0, 0), (60, 60, 60), (NAN, 1.0, NAN), 1),                             # NaN never wins
    ((0, 0), (60, 60), (NAN, NAN), -1),                                        # ... not even alone
    ((0, 0), (60, 60), (-math.inf, -math.inf), -1),                            # nothing is above the start of the search
    ((0, 1), (60, 60), (-5.0, -math.inf), 0),
    ((2, 3), (60, 60), (1.0, 1.0), -1),
    ((1,), (50,), (0.0,), 0),                                                  # exhausted on a coarse level: eligible
    ((1,), (49,), (0.0,), -1),
])
def test_the_selection_rule(statuses, counts, scores, want):
    assert B.select(scores, counts, statuses, 50) == want
    words = B.best_words(want, statuses, counts, len(scores))
    assert words == ([want, statuses[want], counts[want], len(scores)] if want >= 0 else [-1, -1, 0, len(scores)])


# ---- the binding and the argument checks (no device work is reached) -----------------------------------------------------------
def test_the_binding_and_the_scratch_size():
    from sps_amd import _native
    lib = _native.lib
    for name in ("sps_ndt_pyramid_align_batch_scratch", "sps_ndt_pyramid_align_batch"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    assert lib.sps_version() == _native.ABI_VERSION == 202                      # additive: the ABI version does not change
    for cap, k in ((0, 1), (1000, 3), (65536, 64)):
        rows = max(1, (cap + 31) // 32)
        assert lib.sps_ndt_pyramid_align_batch_scratch(cap, k) == k * (rows * 29 * 8 + 8 * 4)
        assert lib.sps_ndt_pyramid_align_batch_scratch(cap, 1) >= lib.sps_ndt_pyramid_align_scratch(cap)
    for cap, k in ((-1, 1), (1000, 0), (1000, 65), (1 << 40, 1)):
        assert lib.sps_ndt_pyramid_align_batch_scratch(cap, k) == -1
    assert lib.sps_ndt_pyramid_align_batch(None, *([None] * 2), 0, None, 1, 0, None, 7, 50, 1e-4, 1e-5, *([None] * 10)) \
        == _native.ERR_INVALID


def bare(**kw):
    """an NDTLocaliser that was never opened: the checks in front of the device work are all it can do"""
    from sps_amd.localiser import NDTLocaliser
    loc = object.__new__(NDTLocaliser)
    for k, v in dict(dict(source="points", resolutions=None, level_capacities=None, cell_capacity=None, resolution=1.0), **kw).items():
        setattr(loc, k, v)
    return loc


def test_python_errors_come_before_any_device_work():
    T = np.eye(4)[None]
    calls = (lambda l, **kw: l.submit_batch(None, 0, T, **kw), lambda l, **kw: l.submit_from_device(None, 0, None, **kw),
             lambda l, **kw: l.relocalise(None, 0, T, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="coarse_to_fine needs a localiser with a pyramid"):
            call(bare(), coarse_to_fine=True)
        with pytest.raises(ValueError, match="coarse_to_fine needs a localiser with a pyramid"):
            call(bare(cell_capacity=64), coarse_to_fine=True, integrate=True)
        with pytest.raises(ValueError, match="source='points'"):               # refused as ever, and first
            call(bare(source="cells"), coarse_to_fine=True)
        # a static pyramid has nothing to integrate into or to carve, with or without the argument
        with pytest.raises(ValueError, match="single-resolution"):
            call(bare(resolutions=(2.0, 1.0)), coarse_to_fine=True, integrate=True)
        with pytest.raises(ValueError, match="single-resolution"):
            call(bare(resolutions=(2.0, 1.0)), coarse_to_fine=True, carve=True)
        # an online pyramid: refused on the single map as ever, accepted coarse to fine (the next check, of the rows, then fails)
        online = dict(resolutions=(2.0, 1.0), level_capacities=(64, 64))
        with pytest.raises(ValueError, match="online map"):
            call(bare(**online), integrate=True)
        with pytest.raises(ValueError, match="online map"):
            call(bare(**online), carve=True)
        with pytest.raises(ValueError, match="max_cell_points"):
            call(bare(**online), coarse_to_fine=True, integrate=True, max_cell_points=-1)
        with pytest.raises(ValueError, match="unknown carve options"):
            call(bare(**online), coarse_to_fine=True, carve=True, carve_options=dict(nonsense=1))
        with pytest.raises(TypeError, match="needs a tensor"):
            call(bare(**online), coarse_to_fine=True, integrate=True, carve=True)
    from sps_amd.localiser import MAX_HYPOTHESES, _checked_poses
    for K in (0, 65):                                                          # the check submit_batch makes of its poses
        with pytest.raises(ValueError, match="1 <= K <= 64"):
            _checked_poses(np.tile(np.eye(4), (K, 1, 1)), "T_inits", MAX_HYPOTHESES, "K")


def test_the_batch_layout_keeps_its_offsets_and_gains_the_level_rows():
    from sps_amd.localiser import _batch_layout
    for K, I, wn, integ, carve in ((1, 30, False, False, False), (5, 7, True, True, False), (64, 3, True, True, True),
                                   (3, 0, False, False, True)):
        old = _batch_layout(K, I, wn, integ, carve)
        assert old["levels"] == old["update"] == old["size"]                   # no level rows without the pyramid
        assert old["carve"] - old["update"] == (2 if integ else 0) and old["total"] - old["carve"] == (2 if carve else 0)
        for L in (None, 3):
            new = _batch_layout(K, I, wn, integ, carve, True, L)
            for name in ("T_out", "status", "n_points", "best", "T_best", "final", "trace", "normal", "size", "hands_on"):
                assert new[name] == old[name], name
            w = 2 if L is None else 2 * L
            assert new["levels"] == old["size"] and new["update"] - new["levels"] == (K * I + 1) // 2
            assert new["carve"] - new["update"] == (w if integ else 0) and new["total"] - new["carve"] == (w if carve else 0)


def test_a_batch_buffer_parses_with_levels_and_per_level_info():
    from sps_amd.localiser import PendingPoses, _batch_layout
    K, I, L = 2, 3, 2
    o = _batch_layout(K, I, False, True, True, True, L)
    h = np.zeros(o["total"])
    h[o["T_out"]:o["status"]] = np.tile(np.eye(4).ravel(), K)
    h[o["status"]:o["n_points"]].view(np.int32)[:] = [0, 3, 70, 1, 2, 1, 0, 0]
    h[o["n_points"]:o["best"]].view(np.int32)[0] = 99
    h[o["best"]:o["T_best"]].view(np.int32)[:] = [0, 0, 70, K]
    h[o["levels"]:o["update"]].view(np.int32)[:K * I] = [0, 0, 1, 0, -1, -1]
    h[o["update"]:o["carve"]].view(np.int32)[:] = np.arange(8)
    h[o["carve"]:o["total"]].view(np.int32)[:] = np.arange(8) + 10
    r = PendingPoses(K, I, False, None, None, None, 0, True, True, True, L)._parse(h)
    assert [list(x.levels) for x in r.results] == [[0, 0, 1], [0]] and [x.iterations for x in r.results] == [3, 1]
    assert [x.status for x in r.results] == [0, 2] and r.best == 0 and r.results[0].n_points == 99
    assert isinstance(r.map_update, tuple) and [u.cells for u in r.map_update] == [0, 4] and r.map_update[1].points == 7
    assert isinstance(r.map_carve, tuple) and [c.rays for c in r.map_carve] == [10, 14]
    # without the pyramid the result is what it was
    o = _batch_layout(K, I, False, True, False)
    r = PendingPoses(K, I, False, None, None, None, 0, True, False)._parse(np.zeros(o["total"]))
    assert r.results[0].levels is None and not isinstance(r.map_update, tuple) and r.map_carve is None


# ---- the loop's options --------------------------------------------------------------------------------------------------------
class TakesPose:
    pass


class TakesNone:
    takes_pose = False


class Est:
    pose_dev = None

    def predict(self, dt): ...
    def predict_imu(self, s): ...
    def correct_from(self, p): ...
    def snapshot(self): ...


class Ndt:
    resolutions = None

    def submit_from_device(self, *a, **k): ...
    def submit_batch(self, *a, **k): ...
    def relocalise(self, *a, **k): ...


class Pyr(Ndt):
    resolutions = (2.0, 1.0)


class OnlinePyr(Pyr):
    level_capacities = (64, 64)


def test_the_loop_options():
    from sps_amd.localiser import LocalisationLoop
    eye, grid = np.eye(4), np.eye(4)[None]
    with pytest.raises(ValueError, match="coarse_to_fine needs a localiser with a pyramid"):
        LocalisationLoop(TakesNone(), Ndt(), eye, coarse_to_fine=True)
    with pytest.raises(ValueError, match="coarse_to_fine needs a localiser with a pyramid"):
        LocalisationLoop(TakesNone(), object(), eye, coarse_to_fine=True)
    # the device path with a pyramid: with coarse_to_fine only, and under the same conditions on the filter as ever
    assert LocalisationLoop(TakesNone(), Pyr(), eye, estimator=Est()).device_guess is False
    with pytest.raises(ValueError, match="device_guess=True needs"):
        LocalisationLoop(TakesNone(), Pyr(), eye, estimator=Est(), device_guess=True)
    assert LocalisationLoop(TakesNone(), Pyr(), eye, estimator=Est(), coarse_to_fine=True).device_guess is True
    assert LocalisationLoop(TakesNone(), Pyr(), eye, estimator=Est(), coarse_to_fine=True, device_guess=True).device_guess is True
    assert LocalisationLoop(TakesNone(), Pyr(), eye, estimator=Est(), coarse_to_fine=True, device_guess=False).device_guess is False
    assert LocalisationLoop(TakesPose(), Pyr(), eye, estimator=Est(), coarse_to_fine=True).device_guess is False
    with pytest.raises(ValueError, match="device_guess=True needs"):
        LocalisationLoop(TakesPose(), Pyr(), eye, estimator=Est(), coarse_to_fine=True, device_guess=True)
    for kw in (dict(hypotheses=grid), dict(search=grid)):
        assert LocalisationLoop(TakesNone(), Pyr(), eye, estimator=Est(), coarse_to_fine=True, **kw).device_guess is False
        with pytest.raises(ValueError, match="device_guess=True needs"):
            LocalisationLoop(TakesNone(), Pyr(), eye, estimator=Est(), coarse_to_fine=True, device_guess=True, **kw)
    with pytest.raises(ValueError, match="device_guess needs an estimator"):
        LocalisationLoop(TakesNone(), Pyr(), eye, coarse_to_fine=True, device_guess=True)
    # an online pyramid: hypotheses and search with the map's update and carve only coarse to fine
    for kw in (dict(hypotheses=grid), dict(search=grid)):
        for op in (dict(update_map=True), dict(carve_map=True)):
            with pytest.raises(ValueError, match="plain registration only"):
                LocalisationLoop(TakesNone(), OnlinePyr(), eye, **kw, **op)
            loop = LocalisationLoop(TakesNone(), OnlinePyr(), eye, coarse_to_fine=True, **kw, **op)
            assert loop.coarse_to_fine is True
    assert LocalisationLoop(TakesNone(), Pyr(), eye).coarse_to_fine is False


class Recorder(Pyr):
    """a pyramid localiser that records how the loop calls it and answers with one converged hypothesis"""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def _answer(self, name, args, kw):
        from sps_amd.localiser import BatchPoseResult, PoseResult, RelocalisationResult
        self.calls.append((name, kw))
        one = PoseResult(np.eye(4), 0, 1, 60, 0.0, np.zeros((1, 4)))
        batch = BatchPoseResult([one], np.zeros(1), np.zeros(1, np.int64), 0, np.eye(4))
        out = dict(submit=one, submit_batch=batch, submit_from_device=batch,
                   relocalise=RelocalisationResult(np.zeros(1), np.zeros(1, np.int64), np.zeros(1, np.int64), batch, 0, np.eye(4)))[name]

        class Done:
            def result(self):
                return out
        return Done()

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
        class Pending:
            def result(self):
                class Result:
                    filtered = scan
                return Result()
        return Pending()


@pytest.mark.parametrize("c2f", [False, True])
def test_the_loop_passes_the_argument_to_the_batch_the_search_and_nothing_else(c2f):
    import torch

    from sps_amd.localiser import LocalisationLoop
    scan, eye, grid = torch.zeros((3, 4)), np.eye(4), np.eye(4)[None]
    extra = dict(coarse_to_fine=True) if c2f else {}
    loc = Recorder()
    LocalisationLoop(HostFilter(), loc, eye, hypotheses=grid, coarse_to_fine=c2f).step(scan)
    assert loc.calls == [("submit_batch", extra)]
    loc = Recorder()
    loop = LocalisationLoop(HostFilter(), loc, eye, search=grid, hypotheses=grid, search_keep=3, coarse_to_fine=c2f)
    loop.step(scan), loop.step(scan)
    assert loc.calls == [("relocalise", dict(extra, keep=3)), ("submit_batch", extra)]
    loc = Recorder()
    LocalisationLoop(HostFilter(), loc, eye, coarse_to_fine=c2f).step(scan)     # the plain registration is the pyramid's already
    assert loc.calls == [("submit", {})]


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_the_driver_option():
    """through click's own runner, in this process: every case ends in the option checks, before any device work"""
    import importlib.util

    from click.testing import CliRunner
    spec = importlib.util.spec_from_file_location("filter_sequence_under_test", os.path.join(ROOT, "scripts", "filter_sequence.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)

    def run(*opts):
        return CliRunner().invoke(script.main, ["--synthetic", "2", "--localise", "--localiser", "ndt", *opts])
    r = CliRunner().invoke(script.main, ["--help"])
    assert r.exit_code == 0 and "--coarse-to-fine" in r.output
    needs = "--coarse-to-fine needs --resolutions and one of --hypotheses, --search, --estimator ukf"
    for opts in (("--coarse-to-fine",), ("--coarse-to-fine", "--hypotheses", "3,1,1"), ("--coarse-to-fine", "--resolutions", "2,1"),
                 ("--coarse-to-fine", "--estimator", "ukf")):
        r = run(*opts)
        assert r.exit_code == 2 and needs in r.output, opts
    # an existing combination keeps its message without the option ...
    r = run("--resolutions", "2,1", "--update-map", "--hypotheses", "3,1,1")
    assert r.exit_code == 2 and "takes no --hypotheses and no --search" in r.output
    # ... and other checks still come where they came
    r = run("--coarse-to-fine", "--resolutions", "2,1", "--hypotheses", "3,1,1", "--level-capacities", "64,64")
    assert r.exit_code == 2 and "--level-capacities needs --update-map or --carve-map" in r.output
