"""CPU tests of distribution-to-distribution NDT registered coarse to fine from several start poses: the
restatement (tests/ndt_d2d_pyramid_batch_reference.py) against K chained single restatements, the scene the GPU test
re-uses, the selection rule, the ``d2d_pyramid=True`` checks that need no device, the frame layout, the loop's routing, the
header, the binding and the drivers' options.  No GPU."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from tests import ndt_d2d_batch_reference as DB
from tests import ndt_d2d_pyramid_batch_reference as R
from tests import ndt_d2d_pyramid_reference as DP
from tests import ndt_d2d_reference as DR
from tests import ndt_pyramid_batch_reference as PB
from tests import ndt_reference as NR
from tests.test_ndt_d2d_batch_cpu import Cells, Est, HostFilter, Points, Recorder, RecordingEst, TakesNone, TakesPose, bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sps_ndt_pyramid_align_d2d_batch_scratch", "sps_ndt_pyramid_align_d2d_batch")


# ---- the scene of the GPU test, on the restatement ------------------------------------------------------------------------------
def test_the_scene_has_a_full_chain_a_skipped_finest_level_and_a_level_0_only():
    assert R.check_scene_properties() == R.CHAIN


@pytest.mark.parametrize("sources,budget", [("all", 0), ("all", 1), ("all", 2), ("all", 3), ("finest skipped", 0),
                                            ("level 0 only", 0)])
def test_the_inputs_mean_something(sources, budget):
    r = R.restated(sources, budget)
    res = r["results"]
    print(f"{sources}, caps and budget {R.BUDGETS[budget]}: status {[x['status'] for x in res]} slots per level "
          f"{[R.slots_per_level(x['levels']) for x in res]} l* {r['level']} scores {np.round(r['scores'], 3)} counts "
          f"{list(r['counts'])} best {r['best']}")
    R.check_input_properties(sources, budget, [x["status"] for x in res], [x["iterations"] for x in res],
                             [x["levels"] for x in res], r["level"])
    # exact counts need an input without a source on a cell face and without a weight on the guard's boundary
    assert all(x["faces"] == 0 and x["boundary"] == 0 for x in res)
    assert all(h["faces"] == 0 and h["boundary"] == 0 for h in r["hits"])
    assert r["best"] not in (-1, R.OFF) and r["words"][3] == 6


# ---- the restatement composes and adds nothing ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sources,budget", [("all", 1), ("finest skipped", 0), ("level 0 only", 0)])
def test_the_batch_is_k_single_restatements_scored_on_the_last_level_of_the_chain(sources, budget):
    sc, r = R.scene(), R.restated(sources, budget)
    srcs, cmaps = sc["src"][sources], sc["cmaps"]
    caps, iters = R.BUDGETS[budget]
    ls = R.CHAIN[sources][-1]
    assert r["level"] == ls
    for k in (0, R.WRONG, R.OFF):
        one = DP.align(srcs, cmaps, R.POSES[k], iters, caps, min_corr=R.MIN_CORR)
        got = r["results"][k]
        assert (got["status"], got["iterations"], got["n_corr"], got["level"]) == (one["status"], one["iterations"],
                                                                                   one["n_corr"], one["level"])
        for name in ("pose", "trace", "normal", "levels"):
            assert got[name].tobytes() == one[name].tobytes(), (k, name)
        s, h = DR.score(srcs[ls], cmaps[ls], one["pose"])
        assert r["scores"][k] == s and r["counts"][k] == len(np.unique(h["i"]))
    assert r["results"][R.OFF]["pose"].tobytes() == R.POSES[R.OFF].tobytes()   # status 2: the start pose comes back
    assert r["best"] == PB.select(r["scores"], r["counts"], [x["status"] for x in r["results"]], R.MIN_CORR)
    assert r["pose"].tobytes() == r["results"][r["best"]]["pose"].tobytes()
    assert r["words"] == [r["best"], r["results"][r["best"]]["status"], r["counts"][r["best"]], 6]


def test_zero_iterations_score_the_start_poses():
    sc = R.scene()
    srcs, cmaps = sc["src"]["finest skipped"], sc["cmaps"]
    r = R.align_batch(srcs, cmaps, R.POSES[:3], iters=0, level_iters=(30, 30, 30))
    assert [x["status"] for x in r["results"]] == [1, 1, 1] and [x["iterations"] for x in r["results"]] == [0, 0, 0]
    assert r["level"] == 1
    for k in range(3):
        assert r["results"][k]["pose"].tobytes() == R.POSES[k].tobytes()
        assert r["scores"][k] == DR.score(srcs[1], cmaps[1], R.POSES[k])[0]


def test_the_scoring_level_follows_min_corr_and_the_capacity():
    srcs = R.scene()["src"]["all"]
    valid = [DP.valid_sources(s) for s in srcs]
    assert valid == [335, 597, 222]
    assert [R.scoring_level(srcs, m) for m in (20, 222, 223, 597, 598)] == [2, 2, 1, 1, 0]
    assert R.scoring_level(srcs, 223, cap_src=222) == 0 and R.scoring_level(srcs, 100, cap_src=100) == 2
    from sps_amd.localiser import _scoring_level
    for m, cap in ((20, 65536), (222, 65536), (223, 65536), (598, 65536), (223, 222), (100, 100), (0, 0)):
        assert _scoring_level(valid, cap, m) == R.scoring_level(srcs, m, cap_src=cap), (m, cap)
    assert _scoring_level([5], 10, 50) == 0 and _scoring_level([-4, -4], 10, 0) == 1   # a count below zero is clipped to 0


# ---- the selection --------------------------------------------------------------------------------------------------------------
def test_selection_on_hand_made_scores():
    sel = DB.select
    assert sel([1.0, 3.0, 3.0], [100] * 3, [0, 1, 0], 20) == 1                # a tie goes to the lowest index
    assert sel([math.nan, 2.0, math.nan], [100] * 3, [0, 0, 0], 20) == 1      # NaN never wins, wherever it stands
    assert sel([math.nan, math.nan], [100] * 2, [0, 0], 20) == -1
    assert sel([1.0, 3.0, 2.0], [100, 19, 20], [0, 0, 0], 20) == 2            # sources counted below min_corr
    assert sel([1.0, 3.0], [100, 100], [2, 3], 20) == -1                      # nobody qualifies
    assert PB.best_words(-1, [2, 3], [100, 100], 2) == [-1, -1, 0, 2] and PB.best_words(1, [0, 1], [7, 9], 2) == [1, 1, 9, 2]


def test_a_tie_and_nobody_qualifying_through_the_batch():
    sc = R.scene()
    srcs, cmaps = sc["src"]["all"], sc["cmaps"]
    twice = R.align_batch(srcs, cmaps, np.stack([R.POSES[2], R.POSES[2], R.POSES[R.OFF]]), 7, (4, 30, 30))
    assert twice["scores"][0] == twice["scores"][1] and twice["best"] == 0 and twice["words"][3] == 3
    off = R.POSES[[R.OFF] * 2].copy()
    off[1, 1, 3] += 1.0
    none = R.align_batch(srcs, cmaps, off, 7, (4, 30, 30))
    assert none["words"] == [-1, -1, 0, 2] and none["pose"].tobytes() == off[0].tobytes()
    # level 0 too sparse: status 2 for every hypothesis after one slot, whatever the finer levels hold
    sparse = R.align_batch(srcs, cmaps, R.POSES[:3], 7, (4, 30, 30), min_corr=336)
    assert [(x["status"], x["iterations"]) for x in sparse["results"]] == [(2, 1)] * 3
    assert sparse["words"] == [-1, -1, 0, 3] and sparse["pose"].tobytes() == R.POSES[0].tobytes() and sparse["level"] == 1
    empty = R.align_batch(srcs, [NR.cells(np.zeros((0, 3)), r) for r in R.RESOLUTIONS], R.POSES[:2], 7, (4, 30, 30))
    assert empty["best"] == -1 and not empty["scores"].any()


# ---- the checks of d2d_pyramid=True that need no device ---------------------------------------------------------------------------
PYR = dict(resolutions=(2.0, 1.0), source_resolutions=(2.0, 1.0))
NEEDS = "d2d_pyramid=True needs an NDTLocaliser with source='cells' and source_resolutions"
ALONE = "d2d_pyramid=True excludes d2d and coarse_to_fine"


def test_d2d_pyramid_refusals_come_before_any_device_work():
    T = np.eye(4)[None]
    calls = dict(submit_batch=lambda l, **kw: l.submit_batch(None, 0, T, **kw),
                 submit_from_device=lambda l, **kw: l.submit_from_device(None, 0, None, **kw),
                 relocalise=lambda l, **kw: l.relocalise(None, 0, T, **kw))
    for name, call in calls.items():
        for loc in (bare(source="points", source_resolutions=None), bare(source_resolutions=None),
                    bare(source="points", resolutions=(2.0, 1.0), source_resolutions=None)):
            with pytest.raises(ValueError, match=NEEDS):
                call(loc, d2d_pyramid=True)
        for extra in (dict(d2d=True), dict(coarse_to_fine=True), dict(d2d=True, coarse_to_fine=True)):
            with pytest.raises(ValueError, match=ALONE):
                call(bare(**PYR), d2d_pyramid=True, **extra)
        # the old pair keeps its refusal and its message, also on a localiser with source_resolutions
        with pytest.raises(ValueError, match="d2d=True and coarse_to_fine exclude each other"):
            call(bare(**PYR), d2d=True, coarse_to_fine=True)
        with pytest.raises(ValueError, match="source='points'"):               # without any keyword: refused as ever
            call(bare(**PYR))
        with pytest.raises(ValueError, match="source='points'"):
            call(bare(**PYR), d2d_pyramid=False)
        with pytest.raises(ValueError, match="online map"):                    # a static pyramid has no map to integrate into
            call(bare(**PYR), d2d_pyramid=True, integrate=True)
        with pytest.raises(ValueError, match="online map"):
            call(bare(**PYR), d2d_pyramid=True, carve=True)
        with pytest.raises(TypeError, match="needs a tensor"):                  # accepted: the next check, of the rows, fails
            call(bare(**PYR), d2d_pyramid=True)
        with pytest.raises(TypeError, match="needs a tensor"):                  # an online pyramid takes the map work
            call(bare(level_capacities=(100, 100), **PYR), d2d_pyramid=True, integrate=True, carve=True)
    for name in ("submit_filtered_batch", "relocalise_filtered"):
        pend = type("Pending", (), dict(_filtered=None, count_dev=None))()
        with pytest.raises(ValueError, match=NEEDS):
            getattr(bare(source_resolutions=None), name)(pend, T, d2d_pyramid=True)
        with pytest.raises(TypeError, match="needs a tensor"):
            getattr(bare(**PYR), name)(pend, T, d2d_pyramid=True)
    for keep in (0, 65):
        with pytest.raises(ValueError, match="keep must be in"):
            bare(**PYR).relocalise(None, 0, T, keep=keep, d2d_pyramid=True)
    for bad in (np.full((2, 4, 4), np.nan), np.zeros((0, 4, 4)), np.eye(4)):
        for name in ("submit_batch", "relocalise"):
            with pytest.raises(ValueError, match="must be finite"):
                getattr(bare(**PYR), name)(None, 0, bad, d2d_pyramid=True)
    with pytest.raises(ValueError, match="1 <= K <= 64"):
        bare(**PYR).submit_batch(None, 0, np.tile(np.eye(4), (65, 1, 1)), d2d_pyramid=True)
    with pytest.raises(ValueError, match="d2d_pyramid=True"):                  # the old refusal names the new keyword
        bare(**PYR).submit_batch(None, 0, T, d2d=True, coarse_to_fine=True)


# ---- the frame layout --------------------------------------------------------------------------------------------------------------
def expected_batch_offsets(K, I, with_normal, integrate, carve, pyramid, L, match, match_words):
    """the layout of a batch's buffer as it was before this keyword, written out by hand, in doubles"""
    w = 2 if L is None else 2 * L
    o, at = {}, 0
    for name, size in (("T_out", 16 * K), ("status", 2 * K), ("n_points", 1), ("best", 2), ("T_best", 16), ("final", 2 * K),
                       ("trace", 4 * K * I), ("normal", 28 * K * I if with_normal else 0)):
        o[name], at = at, at + size
    o["size"] = at
    for name, size in (("levels", (K * I + 1) // 2 if pyramid else 0), ("update", w if integrate else 0),
                       ("carve", w if carve else 0), ("match", match_words if match else 0)):
        o[name], at = at, at + size
    o["total"] = at
    return o


def test_other_localisers_keep_their_layout():
    from sps_amd.localiser import MATCH_WORDS, _batch_layout, _pose_layout
    for K, I in ((1, 0), (1, 30), (5, 7), (64, 90)):
        for with_normal in (False, True):
            for integrate, carve, pyramid, L, match in ((False, False, False, None, False), (True, True, False, None, True),
                                                        (False, False, True, None, False), (True, True, True, 3, True),
                                                        (True, False, True, 4, False)):
                want = expected_batch_offsets(K, I, with_normal, integrate, carve, pyramid, L, match, MATCH_WORDS)
                for got in (_batch_layout(K, I, with_normal, integrate, carve, pyramid, L, match),
                            _batch_layout(K, I, with_normal, integrate, carve, pyramid, L, match, 0)):
                    assert got["sources"] == got["levels"] == want["levels"]  # a part of no words
                    assert {k: got[k] for k in want} == want
                    assert got["hands_on"] == (want["T_best"] * 8, (want["match"] + 4) * 8 if match else want["best"] * 8 + 4)
    # with the sources: L int32 between the hypotheses' rows and the level rows; everything in front stays, the tail moves
    for n_src, words in ((1, 1), (2, 1), (3, 2), (4, 2)):
        a = _batch_layout(5, 7, True, True, True, True, 3, True)
        b = _batch_layout(5, 7, True, True, True, True, 3, True, (n_src, 4096, 20))
        front = ("T_out", "status", "n_points", "best", "T_best", "final", "trace", "normal", "size")
        assert all(a[k] == b[k] for k in front) and b["sources"] == a["size"]
        assert all(b[k] == a[k] + words for k in ("levels", "update", "carve", "match", "total"))
        assert b["hands_on"] == (a["hands_on"][0], a["hands_on"][1] + 8 * words)
    assert _pose_layout(30, True, True, 3, True, True, True, 3)["sources"] == _pose_layout(30, True)["size"]   # submit's, as ever
    with pytest.raises(TypeError):                                             # a batch takes the triple or nothing
        _batch_layout(5, 7, True, True, True, True, 3, True, 3)


def test_a_d2d_pyramid_batch_buffer_parses_with_the_levels_sources():
    from sps_amd.localiser import PendingPoses, _batch_layout
    K, I = 3, 4
    shape = (False, False, True, None, False, (3, 4096, 20))
    o = _batch_layout(K, I, False, *shape)
    h = np.zeros(o["total"])
    h[o["status"]:o["n_points"]].view(np.int32)[:] = [0, 4, 200, 1, 1, 4, 300, 0, 2, 1, 3, 0]
    h[o["n_points"]:o["best"]].view(np.int32)[:] = [4157, 0]
    h[o["best"]:o["T_best"]].view(np.int32)[:] = [0, 0, 200, K]
    h[o["sources"]:o["levels"]].view(np.int32)[:3] = [335, 597, 3]
    h[o["levels"]:o["update"]].view(np.int32)[:K * I] = [0, 0, 1, 1, 0, 0, 0, 0, 0, -1, -1, -1]
    r = PendingPoses(K, I, False, None, None, None, 0, *shape)._parse(h)
    assert (r.score_level, r.n_sources) == (1, 597)                            # 3 valid sources on the finest level: skipped
    assert [(x.n_points, x.n_sources, x.n_corr) for x in r.results] == [(4157, 597, 200), (4157, 335, 300), (4157, 335, 3)]
    assert [list(x.levels) for x in r.results] == [[0, 0, 1, 1], [0, 0, 0, 0], [0]]
    h[o["sources"]:o["levels"]].view(np.int32)[:3] = [335, 19, 3]              # nothing beyond level 0
    r = PendingPoses(K, I, False, None, None, None, 0, *shape)._parse(h)
    assert (r.score_level, r.n_sources) == (0, 335)
    plain = PendingPoses(2, 3, False, None, None, None)._parse(np.zeros(_batch_layout(2, 3, False)["total"]))
    assert plain.score_level is None and plain.n_sources is None               # every other batch: as ever


def test_batch_shape_carries_the_sources_for_this_call_only():
    from sps_amd.localiser import NDTLocaliser
    loc = bare(level_capacities=(100, 100), capacity=4096, min_correspondences=20, _match_opts=None, **PYR)
    shape = NDTLocaliser._batch_shape
    assert shape(loc, True, True, True) == (True, True, True, 2, False)
    assert shape(loc, False, False, False, True) == (False, False, False, None, False)
    assert shape(loc, True, False, True, True) == (True, False, True, 2, False, (2, 4096, 20))


# ---- the loop's routing -----------------------------------------------------------------------------------------------------------
class CellsPyramid(Cells):
    resolutions = (2.0, 1.0)
    source_resolutions = (2.0, 1.0)


class OnlineCellsPyramid(CellsPyramid):
    level_capacities = (100, 100)


class RecorderPyramid(Recorder):
    resolutions = (2.0, 1.0)
    source_resolutions = (2.0, 1.0)


def test_the_loop_options():
    from sps_amd.localiser import LocalisationLoop
    eye, grid = np.eye(4), np.eye(4)[None]
    for loc in (Points(), Cells(), object()):
        with pytest.raises(ValueError, match=NEEDS):
            LocalisationLoop(TakesNone(), loc, eye, d2d_pyramid=True)
    for extra in (dict(d2d=True), dict(coarse_to_fine=True)):
        with pytest.raises(ValueError, match=ALONE):
            LocalisationLoop(TakesNone(), CellsPyramid(), eye, d2d_pyramid=True, **extra)
    with pytest.raises(ValueError, match="d2d=True and coarse_to_fine exclude each other"):   # the old pair: as ever
        LocalisationLoop(TakesNone(), CellsPyramid(), eye, d2d=True, coarse_to_fine=True)
    for kw in (dict(hypotheses=grid), dict(search=grid)):
        with pytest.raises(ValueError, match="source='points'"):               # without the argument: refused as ever
            LocalisationLoop(TakesNone(), CellsPyramid(), eye, **kw)
        loop = LocalisationLoop(TakesNone(), CellsPyramid(), eye, d2d_pyramid=True, **kw)
        assert loop.d2d_pyramid is True and loop.d2d is False and loop.coarse_to_fine is False
        assert LocalisationLoop(TakesNone(), CellsPyramid(), eye, d2d_pyramid=True, estimator=Est(), **kw).device_guess is False
        with pytest.raises(ValueError, match="device_guess=True needs"):
            LocalisationLoop(TakesNone(), CellsPyramid(), eye, d2d_pyramid=True, estimator=Est(), device_guess=True, **kw)
        # an online pyramid is updated and carved by hypotheses and search with the keyword only
        with pytest.raises(ValueError, match="source='points'"):
            LocalisationLoop(TakesNone(), OnlineCellsPyramid(), eye, update_map=True, **kw)
        loop = LocalisationLoop(TakesNone(), OnlineCellsPyramid(), eye, update_map=True, carve_map=True, d2d_pyramid=True, **kw)
        assert loop._kw == dict(integrate=True, max_cell_points=0, carve=True, carve_options=None)
    # the device path: with the keyword only, and under the same conditions on the filter as for points
    assert LocalisationLoop(TakesNone(), CellsPyramid(), eye, estimator=Est()).device_guess is False
    with pytest.raises(ValueError, match="device_guess=True needs"):
        LocalisationLoop(TakesNone(), CellsPyramid(), eye, estimator=Est(), device_guess=True)
    assert LocalisationLoop(TakesNone(), CellsPyramid(), eye, estimator=Est(), d2d_pyramid=True).device_guess is True
    assert LocalisationLoop(TakesNone(), CellsPyramid(), eye, estimator=Est(), d2d_pyramid=True, device_guess=False).device_guess is False
    assert LocalisationLoop(TakesPose(), CellsPyramid(), eye, estimator=Est(), d2d_pyramid=True).device_guess is False
    with pytest.raises(ValueError, match="device_guess=True needs"):
        LocalisationLoop(TakesPose(), CellsPyramid(), eye, estimator=Est(), d2d_pyramid=True, device_guess=True)
    with pytest.raises(ValueError, match="occupancy grid"):                    # recover and the global search stay refused
        LocalisationLoop(TakesNone(), CellsPyramid(), eye, d2d_pyramid=True, recover=dict(after=1, yaw_steps=8))
    assert LocalisationLoop(TakesNone(), Points(), eye).d2d_pyramid is False


def test_the_loop_passes_d2d_pyramid_to_the_batch_the_search_and_the_device_path_and_nothing_else():
    import torch

    from sps_amd.localiser import LocalisationLoop
    scan, eye, grid = torch.zeros((3, 4)), np.eye(4), np.eye(4)[None]
    loc = RecorderPyramid()
    LocalisationLoop(HostFilter(), loc, eye, hypotheses=grid, d2d_pyramid=True).step(scan)
    assert loc.calls == [("submit_batch", dict(d2d_pyramid=True))]
    loc = RecorderPyramid()
    loop = LocalisationLoop(HostFilter(), loc, eye, search=grid, hypotheses=grid, search_keep=3, d2d_pyramid=True)
    loop.step(scan), loop.step(scan)
    assert loc.calls == [("relocalise", dict(d2d_pyramid=True, keep=3)), ("submit_batch", dict(d2d_pyramid=True))]
    loc = RecorderPyramid()
    LocalisationLoop(HostFilter(), loc, eye, d2d_pyramid=True).step(scan)      # the plain registration is on the pyramid already
    assert loc.calls == [("submit", {})]
    loc, est = RecorderPyramid(), RecordingEst()
    loop = LocalisationLoop(HostFilter(), loc, eye, estimator=est, d2d_pyramid=True)
    step = loop.step(scan)
    assert loop.device_guess is True and loc.calls == [("submit_from_device", dict(d2d_pyramid=True))]
    assert len(est.corrected) == 1 and step.batch is not None and not step.flagged
    loc = RecorderPyramid()
    loc.level_capacities = (100, 100)
    LocalisationLoop(HostFilter(), loc, eye, hypotheses=grid, update_map=True, d2d_pyramid=True).step(scan)
    assert loc.calls == [("submit_batch", dict(d2d_pyramid=True, integrate=True, max_cell_points=0))]


# ---- the header, the binding, the drivers ---------------------------------------------------------------------------------------------
def test_the_header_declares_the_two_symbols():
    text = open(os.path.join(ROOT, "include", "sps_hip.h")).read()
    assert "NDT localiser, distribution to distribution, pyramid, several hypotheses" in text
    for name in SYMBOLS:
        assert re.search(r"^int(64_t)? " + name + r"\(", text, re.M), name
    assert re.search(r"int64_t sps_ndt_pyramid_align_d2d_batch_scratch\(int64_t cap_src, int n_hyp\);", text)
    assert re.search(r"int sps_ndt_pyramid_align_d2d_batch\(sps_ctx \*ctx, const double \*src_dev, const int32_t \*n_src_dev, "
                     r"int64_t cap_src,\s+const double \*T_init_dev, int n_hyp, int iters, const int32_t \*level_iters, "
                     r"int neighbours,\s+int min_corr, double tol_t, double tol_r, double \*T_out_dev, int32_t \*status_dev,\s+"
                     r"double \*trace_dev, double \*normal_dev, int32_t \*level_dev, double \*final_dev,\s+"
                     r"int32_t \*best_dev, double \*T_best_dev, void \*scratch_dev, void \*stream\);", text)


def test_the_binding_knows_the_entry_points():
    from sps_amd import _native
    lib = _native.lib
    for name in SYMBOLS:
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert lib.sps_version() == _native.ABI_VERSION == 202                     # additive: the ABI version does not change
    assert lib.sps_ndt_pyramid_align_d2d_batch.argtypes == lib.sps_ndt_pyramid_align_batch.argtypes
    assert lib.sps_ndt_pyramid_align_d2d_batch_scratch(1000, 18) == lib.sps_ndt_pyramid_align_batch_scratch(1000, 18) > 0
    assert lib.sps_ndt_pyramid_align_d2d_batch_scratch(1000, 18) == 18 * 32 * 29 * 8 + 18 * 8 * 4   # 32 rows of 29 terms, 8 state words
    for cap, k in ((-1, 1), (1 << 24, 1), (100, 0), (100, 65)):
        assert lib.sps_ndt_pyramid_align_d2d_batch_scratch(cap, k) == -1


def test_the_binding_passes_its_arguments_in_the_header_s_order(monkeypatch):
    from sps_amd import _native
    seen = {}

    def fake(name):
        def call(*args):
            seen[name] = args
            return 0
        return call
    for name in ("sps_ndt_pyramid_align_d2d_batch", "sps_ndt_pyramid_align_batch"):
        monkeypatch.setattr(_native.lib, name, fake(name))
    ctx = object.__new__(_native.Context)
    ctx.handle = "ctx"
    try:
        args = (101, 102, 4096, 103, 5, 90, (30, 20, 10), 7, 20, 1e-4, 1e-5, 104, 105, 106, None, 107, 108, 109, 110, 111, 112)
        ctx.ndt_pyramid_align_d2d_batch(*args)
        assert list(seen) == ["sps_ndt_pyramid_align_d2d_batch"]
        got = seen["sps_ndt_pyramid_align_d2d_batch"]
        caps = got[7]
        assert isinstance(caps, ctypes.Array) and list(caps) == [30, 20, 10]
        assert got[:7] + got[8:] == ("ctx",) + args[:6] + args[7:]
        ctx.ndt_pyramid_align_batch(*args)                                     # the point call keeps its entry point
        assert list(seen) == ["sps_ndt_pyramid_align_d2d_batch", "sps_ndt_pyramid_align_batch"]
        assert seen["sps_ndt_pyramid_align_batch"][8:] == got[8:]
    finally:
        ctx.handle = None


def load_script(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_driver_option():
    """through click's own runner, in this process: every case ends in the option checks, before any device work"""
    from click.testing import CliRunner
    script = load_script(("scripts", "filter_sequence.py"), "filter_sequence_under_test_d2d_pyramid")

    def run(*opts):
        return CliRunner().invoke(script.main, ["--synthetic", "2", "--localise", "--localiser", "ndt", *opts])
    r = CliRunner().invoke(script.main, ["--help"])
    assert r.exit_code == 0 and "--d2d-pyramid" in r.output
    needs = "--d2d-pyramid needs --source cells, --resolutions, --source-resolutions and one of --hypotheses"
    full = ("--source", "cells", "--resolutions", "2,1", "--source-resolutions", "2,1")
    for opts in (("--d2d-pyramid",), ("--d2d-pyramid", "--hypotheses", "3,1,1"), ("--d2d-pyramid", *full),
                 ("--d2d-pyramid", "--source", "cells", "--hypotheses", "3,1,1"),
                 ("--d2d-pyramid", "--source", "cells", "--resolutions", "2,1", "--estimator", "ukf"),
                 ("--d2d-pyramid", "--resolutions", "2,1", "--search", "3,1,1"),
                 ("--d2d-pyramid", "--coarse-to-fine", *full, "--hypotheses", "3,1,1")):
        r = run(*opts)
        assert r.exit_code == 2 and needs in r.output, (opts, r.output)
    r = run("--d2d-pyramid", "--d2d", *full, "--hypotheses", "3,1,1")
    assert r.exit_code == 2 and "neither --d2d nor --coarse-to-fine" in r.output
    for opts in (("--hypotheses", "3,1,1"), ("--search", "3,1,1")):             # without the flag: the message as ever
        r = run(*full, *opts)
        assert r.exit_code == 2 and "--source cells takes no --resolutions, --hypotheses or --search" in r.output, opts


def test_the_timing_tool_option(monkeypatch, capsys):
    tool = load_script(("tools", "localiser_timing.py"), "localiser_timing_under_test_d2d_pyramid")
    full = ["--localiser", "ndt", "--source", "cells", "--resolutions", "2,1", "--source-resolutions", "2,1"]
    for opts in (["--d2d-pyramid"], ["--d2d-pyramid", "--localiser", "ndt", "--source", "cells"],
                 ["--d2d-pyramid", "--localiser", "ndt", "--resolutions", "2,1"], ["--d2d-pyramid", *full, "--hypotheses", "8"],
                 ["--d2d-pyramid", *full, "--estimator"], ["--d2d-pyramid", *full, "--coarse-to-fine"]):
        monkeypatch.setattr("sys.argv", ["localiser_timing.py", *opts])
        with pytest.raises(SystemExit) as e:
            tool.main()
        assert e.value.code == 2 and "--d2d-pyramid needs" in capsys.readouterr().err, opts
    monkeypatch.setattr("sys.argv", ["localiser_timing.py", *full, "--search", "64"])   # the search needs the flag, as ever
    with pytest.raises(SystemExit) as e:
        tool.main()
    assert e.value.code == 2 and "--source-resolutions needs" in capsys.readouterr().err
    seen = []
    monkeypatch.setattr(tool, "restatement_only", lambda a: seen.append(a))    # accepted: the options pass every check
    monkeypatch.setattr("sys.argv", ["localiser_timing.py", "--d2d-pyramid", *full, "--search", "64", "--cpu-only"])
    tool.main()
    assert len(seen) == 1 and seen[0].d2d_pyramid and seen[0].source_resolutions == (2.0, 1.0) and seen[0].search == 64
