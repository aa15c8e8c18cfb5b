"""CPU tests of the multi-resolution NDT alignment's numpy restatement (tests/ndt_pyramid_reference.py), of the binding, of
the constructor's checks and of the driver's options.  No GPU.  Scene and settings are tests/test_ndt_cpu.py's: 400 x 32
rays, scan 1 thinned at leaf 0.4 (4 157 points), 7 neighbours, 30 iterations per alignment."""
import os
import subprocess
import sys

import numpy as np
import pytest

from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_pyramid_reference as PR
from tests import ndt_reference as NR
from tests.test_ndt_cpu import KW, LEAF, T_TRUE, sensor_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOLUTIONS = (2.0, 1.0, 0.5)


@pytest.fixture(scope="module")
def cmaps():
    return PR.pyramid(synthetic.build_map(**KW)[:, :3].astype(np.float64), RESOLUTIONS)


@pytest.fixture(scope="module")
def pts():
    scan = sensor_scan(1)
    return LR.downsample(scan, len(scan), LEAF)[1]


def along(off):
    """a start pose `off` metres off along the corridor"""
    return LR.perturbation(off, 0.0, 0.0, 0.0) @ T_TRUE


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_the_restatement_is_the_single_alignment_chained(cmaps, pts):
    """level after level with a shared budget: the rows of every level are NR.align's from the pose handed over"""
    r = PR.align(pts, cmaps, along(0.5), iters=90, level_iters=(30, 30, 30))
    T, rows = along(0.5), []
    for l, cm in enumerate(cmaps):
        one = NR.align(pts, cm, T)
        assert one["status"] in (0, 1)
        T = one["pose"]
        rows.append(one)
    assert r["pose"].tobytes() == T.tobytes() and r["status"] == rows[-1]["status"]
    assert list(r["levels"]) == sum(([l] * one["iterations"] for l, one in enumerate(rows)), [])
    assert r["trace"].tobytes() == np.concatenate([one["trace"] for one in rows]).tobytes()
    assert r["normal"].tobytes() == np.concatenate([one["normal"] for one in rows]).tobytes()
    assert (r["iterations"], r["n_corr"], r["level"]) == (len(r["levels"]), rows[-1]["n_corr"], 2)
    # one level is NR.align itself
    single = PR.align(pts, cmaps[1:2], along(0.5))
    one = NR.align(pts, cmaps[1], along(0.5))
    assert single["pose"].tobytes() == one["pose"].tobytes() and single["trace"].tobytes() == one["trace"].tobytes()
    assert (single["status"], single["iterations"]) == (one["status"], one["iterations"]) and not single["levels"].any()


@pytest.mark.parametrize("off", [0.5, 1.0])
def test_the_pyramid_recovers_a_lag_along_the_corridor_that_one_level_does_not(cmaps, pts, off):
    """The 1 m map alone stays more than 0.1 m away (measured 0.143 m from 0.5 m and 0.913 m from 1.0 m); 2 -> 1 -> 0.5 with
    30 slots per level ends within 0.02 m (measured 0.0054 m from both; 0.02 m is the 2 m level's own end error)."""
    assert [int(c["valid"].sum()) for c in cmaps] == [443, 1225, 2996] and len(pts) == 4157
    r = PR.align(pts, cmaps, along(off), iters=90, level_iters=(30, 30, 30))
    one = NR.align(pts, cmaps[1], along(off))
    et, er = LR.pose_difference(r["pose"], T_TRUE)
    ot, _ = LR.pose_difference(one["pose"], T_TRUE)
    per = ", ".join(f"{p['status']}/{p['iterations']}" for p in r["per_level"])
    print(f"start {off} m along: pyramid {et:.4f} m {er:.5f} rad, status {r['status']}, {r['iterations']} slots ({per}); "
          f"1 m map alone {ot:.4f} m, status {one['status']} after {one['iterations']} iterations")
    assert r["status"] in (0, 1) and et < 0.02
    assert ot > 0.1


def test_the_one_and_a_half_metre_lag_is_printed_not_asserted(cmaps, pts):
    r = PR.align(pts, cmaps, along(1.5), iters=90, level_iters=(30, 30, 30))
    one = NR.align(pts, cmaps[1], along(1.5))
    print(f"start 1.5 m along: pyramid {LR.pose_difference(r['pose'], T_TRUE)[0]:.4f} m, "
          f"1 m map alone {LR.pose_difference(one['pose'], T_TRUE)[0]:.4f} m (neither recovers it: the pose search's case)")
    assert r["status"] in (0, 1)


# ---- the budget ------------------------------------------------------------------------------------------------------------
def test_budget_exhaustion(cmaps, pts):
    r = PR.align(pts, cmaps, along(0.5), iters=10, level_iters=(30, 30, 30))
    assert (r["status"], r["iterations"], r["level"]) == (1, 10, 0) and not r["levels"].any()
    r = PR.align(pts, cmaps, along(0.5), iters=90, level_iters=(2, 2, 30))
    assert r["levels"][4] == 2 and r["levels"][4:].min() == 2          # level 2 at slot 4 at the latest
    assert (np.diff(r["levels"]) >= 0).all() and (r["levels"] == 0).sum() <= 2 and (r["levels"] == 1).sum() <= 2
    # a budget that ends inside a later level: status 1 there
    r = PR.align(pts, cmaps, along(0.5), iters=5, level_iters=(2, 2, 30))
    assert (r["status"], r["iterations"], r["level"]) == (1, 5, 2)
    # no budget at all
    r = PR.align(pts, cmaps, along(0.5), iters=0)
    assert (r["status"], r["iterations"]) == (1, 0) and r["pose"].tobytes() == along(0.5).tobytes() and r["trace"].shape == (0, 4)


def test_status_2_is_final_at_any_level(cmaps, pts):
    empty = NR.cells(np.zeros((0, 3)), 2.0)
    r = PR.align(pts, [empty] + cmaps[1:], along(0.5), iters=90)
    assert (r["status"], r["iterations"], r["n_corr"], r["level"]) == (2, 1, 0, 0) and r["pose"].tobytes() == along(0.5).tobytes()
    r = PR.align(pts, cmaps[:2] + [NR.cells(np.zeros((0, 3)), 0.5)], along(0.5), iters=90)
    assert r["status"] == 2 and r["level"] == 2 and r["levels"][-1] == 2 and r["pose"].tobytes() == along(0.5).tobytes()


# ---- the binding, the constructor, the driver ------------------------------------------------------------------------------
def test_the_binding_knows_the_pyramid_entry_points():
    from sps_amd import _native
    for name in ("sps_ndt_pyramid_build", "sps_ndt_pyramid_cells", "sps_ndt_pyramid_align_scratch", "sps_ndt_pyramid_align"):
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
    assert _native.lib.sps_version() == _native.ABI_VERSION                 # additive: the ABI version does not change
    # the partial rows of sps_ndt_align and 8 state words instead of its 4
    assert _native.lib.sps_ndt_pyramid_align_scratch(1000) == _native.lib.sps_ndt_align_scratch(1000) + 16
    assert _native.lib.sps_ndt_pyramid_align_scratch(-1) == -1
    for name in ("ndt_pyramid_build", "ndt_pyramid_cells", "ndt_pyramid_align"):
        assert callable(getattr(_native.Context, name))


def test_constructor_errors_come_before_any_device_work():
    """device="nowhere:0" is never looked at: every one of these is refused first"""
    from sps_amd.localiser import MAX_LEVELS, NDTLocaliser, PoseResult
    mp = np.zeros((10, 3))
    assert MAX_LEVELS == 4
    for kw in (dict(resolutions=(2.0, 1.0), cell_capacity=4096),          # the online map is single-resolution
               dict(resolutions=(1.0, 2.0)), dict(resolutions=(1.0, 1.0)), dict(resolutions=(2.0, float("nan"))),
               dict(resolutions=(2.0, 0.0)), dict(resolutions=()),
               dict(resolutions=(8.0, 4.0, 2.0, 1.0, 0.5)),               # more than 4 levels
               dict(resolutions=(2.0, 1.0), level_iterations=(30,)),       # the wrong length
               dict(resolutions=(2.0, 1.0), level_iterations=(30, 0)),     # an entry below 1
               dict(level_iterations=(30,))):                              # no pyramid to cap
        with pytest.raises(ValueError):
            NDTLocaliser(mp, device="nowhere:0", **kw)
    # integrate on a pyramid localiser: refused by the check every submit makes first
    loc = object.__new__(NDTLocaliser)
    loc.resolutions, loc.cell_capacity = (2.0, 1.0), None
    with pytest.raises(ValueError, match="single-resolution"):
        loc._check_integrate(True)
    with pytest.raises(ValueError, match="single-resolution"):
        loc.submit(None, 0, np.eye(4), integrate=True)
    loc._check_integrate(False)
    assert PoseResult(np.eye(4), 0, 0, 0, 0.0, np.zeros((0, 4))).levels is None


def test_the_driver_lists_the_pyramid_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "filter_sequence.py"), "--help"], capture_output=True,
                       text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-1500:]
    assert "--resolutions" in r.stdout and "--level-iterations" in r.stdout
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "filter_sequence.py"), "--synthetic", "2", "--localise", "--resolutions", "2,1"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--resolutions needs --localise --localiser ndt" in r.stderr
