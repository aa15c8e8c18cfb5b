"""CPU tests of the NDT localiser's numpy restatement (tests/ndt_reference.py), of the hand-built map cells the GPU test
re-uses, and of the driver's --localiser option.  No GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_reference as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(n_azimuth=400, n_beams=32)
LEAF = 0.4
T_TRUE = LR.perturbation(0.8, -0.3, 0.05, 20.0)
# the start pose of tests/test_hip_ndt.py: 0.3 m / 2 degrees off, the ICP test's own.  The restatement converges from
# it (test_the_restatement_converges_on_the_gpu_tests_input), so it was not shrunk.
T_INIT = LR.perturbation(0.2, 0.2, 0.1, 2.0) @ T_TRUE


def sensor_scan(seed, T_true=T_TRUE):
    world = synthetic.lidar_scan(seed, **KW)
    Ti = np.linalg.inv(T_true)
    xyz = world[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]
    return np.c_[xyz, world[:, 3]].astype(np.float32)


@pytest.fixture(scope="module")
def cmap():
    return NR.cells(synthetic.build_map(**KW)[:, :3].astype(np.float64), 1.0)


@pytest.fixture(scope="module")
def pts():
    scan = sensor_scan(1)
    return LR.downsample(scan, len(scan), LEAF)[1]


# ---- the gradient and the Hessian ------------------------------------------------------------------------------------------
def test_gradient_equals_the_finite_difference_of_the_score(cmap, pts):
    """g is the gradient of the function the step minimises, f = -score, with respect to the left-multiplied twist
    (omega, v): g_k = -d score / d xi_k.  Central differences D(h) = (score(+h e_k) - score(-h e_k)) / 2h obey
    D(h) = score' + C h^2 + O(h^4), so the truncation error of D(h) is |D(2h) - D(h)| / 3 to leading order; the rounding
    error is that of two sums of m terms (each math.fsum-exact, the terms themselves good to ~8 roundings of 2^-53 and
    two exp calls of <= 1 ulp: 12 * 2^-53 relative is generous) divided by 2h.  The tolerance is 4 x the first plus the
    second, nothing is fitted to the outcome."""
    sub = pts[::7]
    h = 1e-4
    f0, h0 = NR.score(sub, cmap, T_INIT)
    assert len(h0["i"]) > 300 and h0["faces"] == 0
    d1, d2 = NR.gauss(0.55, 1.0)
    g = np.array([math.fsum(h0["terms"][:, 21 + k]) for k in range(6)])
    for k in range(6):
        D = {}
        for step in (h, 2 * h):
            xi = np.zeros(6)
            xi[k] = step
            fp, hp = NR.score(sub, cmap, NR.twist_pose(xi, T_INIT))
            fm, hm = NR.score(sub, cmap, NR.twist_pose(-xi, T_INIT))
            # the score is smooth only while every point keeps its cells
            assert np.array_equal(hp["i"], h0["i"]) and np.array_equal(hp["c"], h0["c"])
            assert np.array_equal(hm["i"], h0["i"]) and np.array_equal(hm["c"], h0["c"])
            D[step] = (fp - fm) / (2 * step)
        trunc = abs(D[2 * h] - D[h]) / 3.0
        rounding = 12 * 2.0 ** -53 * 2 * abs(f0) / (2 * h)
        tol = 4 * trunc + rounding
        print(f"twist {k}: g {g[k]:+.9e}  -D(h) {-D[h]:+.9e}  |diff| {abs(g[k] + D[h]):.3e}  tol {tol:.3e}")
        assert abs(g[k] + D[h]) <= tol, k


def test_hessian_is_symmetric_and_positive_semidefinite(cmap, pts):
    r = NR.align(pts, cmap, T_INIT, iters=1)
    tot = r["normal"][0]
    H = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = tot[k]
            k += 1
    # every per-cell block a J^T icov J is PSD on its own (a >= 0, icov = V diag(1 / lambda) V^T with lambda > 0): check
    # the blocks' quadratic forms on the unit vectors and a fixed set of directions, and the sum's eigenvalues
    terms = r["terms"][0]
    assert (terms[:, [0, 6, 11, 15, 18, 20]] >= 0.0).all()              # the diagonals of every block
    lam = np.linalg.eigvalsh(H)
    print("eigenvalues of H:", lam)
    assert lam.min() >= -1e-12 * lam.max()
    assert np.array_equal(H, H.T)


# ---- hand-built cells ------------------------------------------------------------------------------------------------------
def test_hand_built_cells():
    hb, names = NR.hand_built_cells()
    cm = NR.cells(hb, 1.0, min_points=6, eig_ratio=0.01)
    row = {k: NR.find_cell(cm, v) for k, v in names.items()}
    assert cm["count"][row["five"]] == 5 and not cm["valid"][row["five"]]
    assert cm["count"][row["six"]] == 6 and cm["valid"][row["six"]]
    assert cm["count"][row["same"]] == 6 and not cm["valid"][row["same"]]
    assert (cm["cov"][row["same"]] == 0.0).all()
    p = row["plane"]
    assert cm["count"][p] == 6 and cm["valid"][p]
    lam = np.sort(cm["lam"][p])
    assert lam[0] == 0.01 * lam[2] and lam[1] > lam[0]                    # the flat direction is floored, exactly
    # the floored direction is z: icov's zz entry is 1 / (0.01 lambda_max)
    assert cm["icov"][p][5] == pytest.approx(1.0 / lam[0], rel=1e-12)
    # x = -0.3 at resolution 1 lies in cell -1: floor, not truncation
    assert list(names["neg"]) == [-1, 200, 50]
    assert list(NR.cell_index(np.array([-0.3, 0.3, -1.0]), 1.0)) == [-1, 0, -1]
    assert cm["count"][row["neg"]] == 1 and not cm["valid"][row["neg"]]
    # the two eigen-decomposition routes agree on which cells are valid and on the floored cell
    ce = NR.cells(hb, 1.0, route="eigh")
    assert np.array_equal(ce["valid"], cm["valid"])
    np.testing.assert_allclose(ce["icov"][p], cm["icov"][p], rtol=1e-10, atol=1e-10 * abs(cm["icov"][p]).max())


def test_min_points_and_eig_ratio_are_respected():
    hb, names = NR.hand_built_cells()
    cm = NR.cells(hb, 1.0, min_points=5, eig_ratio=0.1)
    assert cm["valid"][NR.find_cell(cm, names["five"])]
    lam = np.sort(cm["lam"][NR.find_cell(cm, names["plane"])])
    assert lam[0] == 0.1 * lam[2]


def test_gauss_constants():
    d1, d2 = NR.gauss(0.55, 1.0)
    c1, c2 = 4.5, 0.55
    assert d1 == pytest.approx(-math.log(c1 + c2) + math.log(c2), rel=1e-15)
    assert d1 < 0 < d2 < 1                                               # so w = d2 exp(.) never reaches the guard's 1
    # the fit reproduces the mixture at s = 0 and s = 1:  -log(c1 exp(-s / 2) + c2) = d1 exp(-d2 s / 2) + d3
    d3 = -math.log(c2)
    for s in (0.0, 1.0):
        assert d1 * math.exp(-d2 * s / 2) + d3 == pytest.approx(-math.log(c1 * math.exp(-s / 2) + c2), rel=1e-12)


# ---- the whole alignment ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("neighbours", [7, 1])
def test_the_restatement_converges_on_the_gpu_tests_input(cmap, pts, neighbours):
    r = NR.align(pts, cmap, T_INIT, neighbours=neighbours)
    et, er = LR.pose_difference(r["pose"], T_TRUE)
    print(f"neighbours {neighbours}: status {r['status']} after {r['iterations']} iterations, {r['n_corr']} points, "
          f"error {et:.4f} m {er:.5f} rad; score per iteration {np.round(r['trace'][:, 1], 1)}")
    assert r["status"] == 0 and r["iterations"] < 30
    e0t, e0r = LR.pose_difference(T_INIT, T_TRUE)
    assert et < 0.1 * e0t and er < 0.1 * e0r                              # well inside the basin: >10 x closer than the start
    assert r["trace"][-1, 1] > r["trace"][0, 1]                           # the score went up


def test_an_empty_map_and_a_scan_off_the_map_end_with_status_2(cmap, pts):
    empty = NR.cells(np.zeros((0, 3)), 1.0)
    r = NR.align(pts, empty, T_INIT)
    assert (r["status"], r["iterations"], r["n_corr"]) == (2, 1, 0) and r["pose"].tobytes() == T_INIT.tobytes()
    far = pts + [500.0, 0.0, 0.0]
    r = NR.align(far, cmap, T_INIT)
    assert r["status"] == 2 and r["pose"].tobytes() == T_INIT.tobytes()


# ---- the driver ------------------------------------------------------------------------------------------------------------
def test_localiser_option_needs_localise():
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "filter_sequence.py"), "--synthetic", "2", "--localiser", "ndt"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2, r.stdout[-500:] + r.stderr[-1500:]
    assert "--localiser needs --localise" in r.stderr


def test_the_binding_knows_the_ndt_entry_points():
    from sps_amd import _native
    for name in ("sps_ndt_align_scratch", "sps_ndt_map_build", "sps_ndt_map_cells", "sps_ndt_align"):
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
    assert _native.lib.sps_version() == _native.ABI_VERSION == 202        # additive: the ABI version does not change
    assert _native.lib.sps_ndt_align_scratch(1000) == _native.lib.sps_loc_align_scratch(1000) > 0
    assert _native.lib.sps_ndt_align_scratch(-1) == -1
