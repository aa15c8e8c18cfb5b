"""CPU tests of the numpy restatement of distribution-to-distribution NDT registered coarse to fine
(tests/ndt_d2d_pyramid_reference.py), of the binding, of the constructor's checks and of the drivers' options.  No GPU.
Scene and settings are tests/test_ndt_cpu.py's: 400 x 32 rays, scan 1 thinned at leaf 0.4 (4 157 points), 7 neighbours,
and min_corr = 20; map and sources at 2 / 1 / 0.5 m."""
import os
import subprocess
import sys

import numpy as np
import pytest

from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_d2d_pyramid_reference as DP
from tests import ndt_d2d_reference as DR
from tests import ndt_reference as NR
from tests.test_ndt_cpu import KW, LEAF, T_TRUE, sensor_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOLUTIONS = (2.0, 1.0, 0.5)
MIN_CORR = 20
KWA = dict(min_corr=MIN_CORR)


@pytest.fixture(scope="module")
def cmaps():
    return DP.pyramid(synthetic.build_map(**KW)[:, :3].astype(np.float64), RESOLUTIONS)


@pytest.fixture(scope="module")
def pts():
    scan = sensor_scan(1)
    return LR.downsample(scan, len(scan), LEAF)[1]


@pytest.fixture(scope="module")
def srcs(pts):
    """the scan's cells of the three levels at source_min_points 6 and 3"""
    return {mp: DP.sources(pts, RESOLUTIONS, mp) for mp in (6, 3)}


def along(off):
    """a start pose `off` metres off along the corridor"""
    return LR.perturbation(off, 0.0, 0.0, 0.0) @ T_TRUE


def slots(r, L=3):
    return [int((r["levels"] == l).sum()) for l in range(L)]


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_the_sources_of_a_level_are_the_single_build_at_its_resolution(pts, srcs):
    assert [s["n_src"] for s in srcs[6]] == [(443, 202), (1227, 246), (2872, 3)]
    assert [s["n_src"] for s in srcs[3]] == [(443, 335), (1227, 597), (2872, 222)]
    mixed = DP.sources(pts, (2.0, 2.0, 0.5), (6, 3, 3))                   # per-level min_points; equal resolutions are legal
    for s, (r, m) in zip(mixed, ((2.0, 6), (2.0, 3), (0.5, 3))):
        one = DR.sources(pts, r, m)
        assert DR.records(s).tobytes() == DR.records(one).tobytes() and s["n_src"] == one["n_src"]
    assert mixed[0]["n_src"] == (443, 202) and mixed[1]["n_src"] == (443, 335)


def test_the_restatement_is_the_single_alignment_chained(cmaps, srcs):
    """level after level with a shared budget: the rows of every level are DR.align's from the pose handed over"""
    S = srcs[3]
    r = DP.align(S, cmaps, along(0.5), iters=90, level_iters=(30, 30, 30), **KWA)
    T, rows = along(0.5), []
    for s, cm in zip(S, cmaps):
        one = DR.align(s, cm, T, **KWA)
        assert one["status"] in (0, 1)
        T = one["pose"]
        rows.append(one)
    assert r["pose"].tobytes() == T.tobytes() and r["status"] == rows[-1]["status"] and r["entered"] == [0, 1, 2]
    assert list(r["levels"]) == sum(([l] * one["iterations"] for l, one in enumerate(rows)), [])
    assert r["trace"].tobytes() == np.concatenate([one["trace"] for one in rows]).tobytes()
    assert r["normal"].tobytes() == np.concatenate([one["normal"] for one in rows]).tobytes()
    assert (r["iterations"], r["n_corr"], r["level"], r["n_sources"]) == (len(r["levels"]), rows[-1]["n_corr"], 2, 222)
    # one level is DR.align itself
    single = DP.align(S[1:2], cmaps[1:2], along(0.5), **KWA)
    one = DR.align(S[1], cmaps[1], along(0.5), **KWA)
    assert single["pose"].tobytes() == one["pose"].tobytes() and single["trace"].tobytes() == one["trace"].tobytes()
    assert (single["status"], single["iterations"]) == (one["status"], one["iterations"]) and not single["levels"].any()


@pytest.mark.parametrize("mp,off,single_status,pyr_slots,pyr_level", [
    (6, 0.5, 0, [10, 10, 0], 1), (6, 1.0, 1, [17, 10, 0], 1), (3, 0.5, 0, [10, 8, 5], 2), (3, 1.0, 0, [17, 8, 5], 2)])
def test_the_pyramid_recovers_a_lag_along_the_corridor_that_one_level_does_not(cmaps, srcs, mp, off, single_status, pyr_slots,
                                                                                pyr_level):
    """The table of DESIGN.md 8p.  1 m cells alone from 1.0 m with min_points 3 end with status 0 more than 0.5 m away; the
    pyramid ends within a sanity cap of 0.05 m (not a fit: 0.0045 m and 0.0179 m).  At min_points 6 the finest level has 3
    valid sources of 2 872 cells: it is skipped and the call ends with status 0 at level 1."""
    S = srcs[mp]
    one = DR.align(S[1], cmaps[1], along(off), **KWA)
    r = DP.align(S, cmaps, along(off), iters=90, level_iters=(30, 30, 30), **KWA)
    e1, ep = LR.pose_difference(one["pose"], T_TRUE)[0], LR.pose_difference(r["pose"], T_TRUE)[0]
    print(f"min_points {mp}, start {off} m along: 1 m alone {e1:.4f} m status {one['status']} after {one['iterations']}; "
          f"pyramid {ep:.4f} m status {r['status']} slots {slots(r)} sources {r['n_sources']}")
    assert one["status"] == single_status
    assert (r["status"], r["level"], slots(r)) == (0, pyr_level, pyr_slots)
    assert ep < 0.05
    assert r["faces"] == 0 and r["boundary"] == 0
    if off == 1.0:
        assert e1 > 0.5                                                   # status 0 at min_points 3: converged, and wrong
    if mp == 6:
        assert r["entered"] == [0, 1] and r["n_sources"] == 246 and S[2]["n_src"][1] == 3 < MIN_CORR


def test_budget_caps_and_no_slots(cmaps, srcs):
    S = srcs[3]
    r = DP.align(S, cmaps, along(0.5), iters=12, level_iters=(30, 30, 30), **KWA)      # the budget ends inside level 1
    assert (r["status"], slots(r), r["level"], r["n_sources"]) == (1, [10, 2, 0], 1, 597)
    r = DP.align(S, cmaps, along(0.5), iters=10, level_iters=(30, 30, 30), **KWA)      # level 0 converges in the last slot
    assert (r["status"], slots(r), r["level"]) == (1, [10, 0, 0], 0)
    r = DP.align(S, cmaps, along(0.5), iters=90, level_iters=(2, 2, 30), **KWA)        # both handoffs forced by the caps
    assert slots(r)[:2] == [2, 2] and r["status"] == 0 and r["level"] == 2
    r = DP.align(S, cmaps, along(0.5), iters=3, level_iters=(1, 1, 1), **KWA)
    assert (r["status"], slots(r)) == (1, [1, 1, 1])
    r = DP.align(S, cmaps, along(0.5), iters=5, level_iters=(2, 2, 30), **KWA)
    assert (r["status"], slots(r)) == (1, [2, 2, 1])
    r = DP.align(S, cmaps, along(0.5), iters=0, **KWA)
    assert (r["status"], r["iterations"]) == (1, 0) and r["pose"].tobytes() == along(0.5).tobytes() and r["trace"].shape == (0, 4)


def test_the_skip_rule(cmaps, srcs):
    S = srcs[3]
    few = lambda s: dict(s, valid=np.zeros_like(s["valid"]), n_src=(s["n_src"][0], 0))
    # a skipped middle level: level 0 hands over to level 2
    r = DP.align([S[0], few(S[1]), S[2]], cmaps, along(0.5), iters=90, level_iters=(30, 30, 30), **KWA)
    assert r["entered"] == [0, 2] and slots(r)[1] == 0 and r["status"] == 0 and r["level"] == 2
    # nothing qualifies beyond level 0: the coarsest level acts as last, its convergence is status 0 and its cap status 1
    only0 = [S[0], few(S[1]), few(S[2])]
    r = DP.align(only0, cmaps, along(0.5), iters=90, level_iters=(30, 30, 30), **KWA)
    one = DR.align(S[0], cmaps[0], along(0.5), **KWA)
    assert (r["status"], r["entered"], r["n_sources"]) == (0, [0], 335) and r["pose"].tobytes() == one["pose"].tobytes()
    r = DP.align(only0, cmaps, along(0.5), iters=90, level_iters=(3, 30, 30), **KWA)
    assert (r["status"], slots(r)) == (1, [3, 0, 0])
    # the count that decides is the valid one clipped to cap_src
    r = DP.align(S, cmaps, along(0.5), iters=90, level_iters=(30, 30, 30), cap_src=MIN_CORR - 1, **KWA)
    assert r["entered"] == [0]
    # min_corr between the levels' counts: 335 / 597 / 222
    r = DP.align(S, cmaps, along(0.5), iters=90, level_iters=(30, 30, 30), min_corr=223)
    assert r["entered"] == [0, 1] and r["status"] == 0


def test_a_sparse_level_0_ends_with_status_2_after_one_slot(cmaps, srcs):
    """Level 0 is always entered: where it has fewer than min_corr sources the call ends as the single alignment does."""
    S = srcs[6]
    r = DP.align(S, cmaps, along(0.5), iters=90, min_corr=203)            # level 0 has 202 valid sources
    assert (r["status"], r["iterations"], r["level"]) == (2, 1, 0) and r["pose"].tobytes() == along(0.5).tobytes()
    assert r["n_corr"] < 203
    # status 2 at a fine level whose map has no cells: final, and the first start pose comes back
    r = DP.align(srcs[3], cmaps[:2] + [NR.cells(np.zeros((0, 3)), 0.5)], along(0.5), iters=90, **KWA)
    assert r["status"] == 2 and r["level"] == 2 and r["levels"][-1] == 2 and r["pose"].tobytes() == along(0.5).tobytes()


# ---- the constructor, the binding, the drivers ----------------------------------------------------------------------------
def test_source_pyramid_arguments_are_checked_before_any_device_work():
    from sps_amd.localiser import NDTLocaliser
    m = np.zeros((4, 3))
    nd = dict(device="no-such-device")
    with pytest.raises(ValueError, match="source='cells' and resolutions exclude each other"):   # today's message stays
        NDTLocaliser(m, source="cells", resolutions=(2.0, 1.0), **nd)
    with pytest.raises(ValueError, match="source_resolutions needs source='cells' and resolutions"):
        NDTLocaliser(m, resolutions=(2.0, 1.0), source_resolutions=(2.0, 1.0), **nd)
    with pytest.raises(ValueError, match="source_resolutions needs source='cells' and resolutions"):
        NDTLocaliser(m, source="cells", source_resolutions=(2.0, 1.0), **nd)
    with pytest.raises(ValueError, match="exclude each other"):
        NDTLocaliser(m, source="cells", resolutions=(2.0, 1.0), source_resolutions=(2.0, 1.0), source_resolution=1.0, **nd)
    for bad in ((2.0,), (2.0, 1.0, 0.5), (2.0, 0.0), (2.0, float("nan")), (2.0, float("inf")), (2.0, -1.0)):
        with pytest.raises(ValueError, match="one finite entry > 0 per level"):
            NDTLocaliser(m, source="cells", resolutions=(2.0, 1.0), source_resolutions=bad, **nd)
    with pytest.raises(ValueError, match="sequence needs source_resolutions"):
        NDTLocaliser(m, source="cells", source_min_points=(6, 3), **nd)
    for bad in ((6,), (6, 3, 3), (6, -1)):
        with pytest.raises(ValueError, match="one entry >= 0 per level"):
            NDTLocaliser(m, source="cells", resolutions=(2.0, 1.0), source_resolutions=(2.0, 1.0), source_min_points=bad, **nd)
    with pytest.raises(ValueError, match="capacity"):
        NDTLocaliser(m, source="cells", resolutions=(2.0, 1.0), source_resolutions=(2.0, 1.0), capacity=1 << 17, **nd)
    with pytest.raises(ValueError, match="global_grid searches with points"):
        NDTLocaliser(m, source="cells", resolutions=(2.0, 1.0), source_resolutions=(2.0, 1.0), global_grid={}, **nd)
    # what passes the checks: the levels' settings as tuples, equal source resolutions, any order; level_capacities too
    ok = NDTLocaliser._checked_source_pyramid("cells", None, (1.0, 1.0, 3.0), (6, 3, 0), 6, (2.0, 1.0, 0.5))
    assert ok == ((1.0, 1.0, 3.0), (6, 3, 0), None)
    assert NDTLocaliser._checked_source_pyramid("cells", None, (2.0, 1.0), None, 5, (2.0, 1.0)) == ((2.0, 1.0), (5, 5), None)
    assert NDTLocaliser._checked_source_pyramid("cells", None, (2.0, 1.0), 3, 5, (2.0, 1.0)) == ((2.0, 1.0), (3, 3), 3)
    assert NDTLocaliser._checked_source_pyramid("cells", 0.5, None, 4, 6, None) == (None, None, 4)


def test_the_batch_and_the_search_still_refuse_the_pyramid_with_cells():
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser
    loc = object.__new__(NDTLocaliser)                                   # the refusals look at nothing but these
    loc.source, loc.resolutions, loc.source_resolutions = "cells", (2.0, 1.0), (2.0, 1.0)
    rows = np.zeros((1, 4), np.float32)
    for call in (lambda: loc.submit_batch(rows, 1, np.eye(4)[None], d2d=True, coarse_to_fine=True),
                 lambda: loc.submit_from_device(rows, 1, None, d2d=True, coarse_to_fine=True),
                 lambda: loc.relocalise(rows, 1, np.eye(4)[None], d2d=True, coarse_to_fine=True)):
        with pytest.raises(ValueError, match="d2d=True and coarse_to_fine exclude each other"):
            call()
    with pytest.raises(ValueError, match="d2d=True and coarse_to_fine exclude each other"):
        LocalisationLoop(None, loc, np.eye(4), hypotheses=np.eye(4)[None], d2d=True, coarse_to_fine=True)
    with pytest.raises(ValueError, match="source='points'"):
        LocalisationLoop(None, loc, np.eye(4), hypotheses=np.eye(4)[None])
    loop = LocalisationLoop(None, loc, np.eye(4))                        # the plain loop takes such a localiser as it is
    assert not loop.device_guess and not loop.d2d and not loop.coarse_to_fine


def test_the_frame_layout_carries_one_source_count_per_level():
    from sps_amd.localiser import _pose_layout
    base = _pose_layout(30, True, True, None, False, False, True)
    for L in (1, 3, 4):
        o = _pose_layout(30, True, True, None, False, False, True, L)
        assert o["sources"] == base["size"] == o["size"] and o["levels"] - o["sources"] == (L + 1) // 2
        assert o["total"] - base["total"] == (L + 1) // 2 and o["hands_on"][0] == base["hands_on"][0]
    assert _pose_layout(30, True, True, None, False, False, True, 0) == dict(base, sources=base["size"])


def test_the_binding_knows_the_d2d_pyramid_entry_points():
    from sps_amd import _native
    for name in ("sps_ndt_pyramid_source_scratch", "sps_ndt_pyramid_source_build", "sps_ndt_pyramid_align_d2d_scratch",
                 "sps_ndt_pyramid_align_d2d"):
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
    assert _native.lib.sps_version() == _native.ABI_VERSION == 202        # additive: the ABI version does not change
    assert _native.lib.sps_ndt_pyramid_align_d2d_scratch(1000) == _native.lib.sps_ndt_pyramid_align_scratch(1000) > 0
    one = _native.lib.sps_ndt_pyramid_source_scratch(1000, 1)
    assert 0 < one < _native.lib.sps_ndt_pyramid_source_scratch(1000, 3) < 3 * one + 4096
    assert _native.lib.sps_ndt_pyramid_source_scratch(65536, 4) > 0
    for cap, L in ((65537, 1), (-1, 1), (1000, 0), (1000, 5)):
        assert _native.lib.sps_ndt_pyramid_source_scratch(cap, L) == -1
    assert _native.lib.sps_ndt_pyramid_align_d2d_scratch(-1) == -1


def test_the_single_source_scratch_is_the_pyramid_s_for_one_level():
    """one level of the pyramid of sources is the single build's layout, so the two size the same scratch"""
    from sps_amd import _native
    for cap in (0, 1, 255, 256, 257, 65536):
        assert _native.lib.sps_ndt_source_scratch(cap) == _native.lib.sps_ndt_pyramid_source_scratch(cap, 1) > 0
    for cap in (-1, 65537):
        assert _native.lib.sps_ndt_source_scratch(cap) == _native.lib.sps_ndt_pyramid_source_scratch(cap, 1) == -1


def test_the_drivers_list_the_source_pyramid_options():
    for script in (("scripts", "filter_sequence.py"), ("tools", "localiser_timing.py")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, *script), "--help"], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-1500:]
        assert "--source-resolutions" in r.stdout and "--source-min-points" in r.stdout
    fs = [sys.executable, os.path.join(ROOT, "scripts", "filter_sequence.py"), "--synthetic", "2", "--localise", "--localiser", "ndt"]
    r = subprocess.run(fs + ["--source", "cells", "--resolutions", "2,1"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--source cells takes no --resolutions" in r.stderr          # kept without the new option
    r = subprocess.run(fs + ["--resolutions", "2,1", "--source-resolutions", "2,1"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--source-resolutions needs --source cells and --resolutions" in r.stderr
    r = subprocess.run(fs + ["--source", "cells", "--source-min-points", "6,3"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "a --source-min-points list needs --source-resolutions" in r.stderr
    lt = [sys.executable, os.path.join(ROOT, "tools", "localiser_timing.py"), "--localiser", "ndt"]
    r = subprocess.run(lt + ["--source", "cells", "--resolutions", "2,1"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--source cells needs --localiser ndt and none of the other modes" in r.stderr
    r = subprocess.run(lt + ["--resolutions", "2,1", "--source-resolutions", "2,1"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--source-resolutions needs --localiser ndt --source cells --resolutions" in r.stderr
