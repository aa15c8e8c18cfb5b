"""CPU tests of the numpy restatement of distribution-to-distribution NDT (tests/ndt_d2d_reference.py), of the hand-built
source cells the GPU test re-uses, and of the argument checks and driver options that need no device.  No GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_d2d_reference as DR
from tests import ndt_reference as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(n_azimuth=400, n_beams=32)
T_TRUE = LR.perturbation(0.8, -0.3, 0.05, 20.0)
T_INIT = LR.perturbation(0.2, 0.2, 0.1, 2.0) @ T_TRUE                  # the start pose of tests/test_ndt_cpu.py
EIG_RATIO = 0.01
U = 2.0 ** -52


def sensor_scan(seed, T_true=T_TRUE):
    world = synthetic.lidar_scan(seed, **KW)
    Ti = np.linalg.inv(T_true)
    xyz = world[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]
    return np.c_[xyz, world[:, 3]].astype(np.float32)


@pytest.fixture(scope="module")
def cmap():
    return NR.cells(synthetic.build_map(**KW)[:, :3].astype(np.float64), 1.0)


@pytest.fixture(scope="module")
def thinned():
    scan = sensor_scan(1)
    return {leaf: LR.downsample(scan, len(scan), leaf)[1] for leaf in (0.2, 0.4)}


@pytest.fixture(scope="module")
def srcs(thinned):
    return {leaf: DR.sources(p, 1.0, 6, EIG_RATIO) for leaf, p in thinned.items()}


def every_third(src):
    """the sub-sample of the gradient test: every third valid source (checked below to keep its cells across the steps)"""
    keep = np.zeros(len(src["valid"]), bool)
    keep[np.nonzero(src["valid"])[0][::3]] = True
    return dict(src, valid=keep)


def full_H(tot):
    H = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = tot[k]
            k += 1
    return H


# ---- 1. the gradient -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", [True, False])
def test_gradient_equals_the_finite_difference_of_the_frozen_score(cmap, srcs, frozen):
    """g is the gradient of f = -score with B held at the current pose.  With R_frozen = the rotation of the pose, Cw and
    so B do not move with the twist and all six components of g equal the central difference; without freezing the three
    translation components still do, since B does not depend on t.  The tolerance is built as in
    test_ndt_cpu.test_gradient_equals_the_finite_difference_of_the_score: 4 x the truncation estimate |D(2h) - D(h)| / 3
    plus the rounding term.  The rounding of a term is here that of the point path (12 * 2^-53 relative) plus that of
    s = x . B x through the two inverses of a matrix of condition <= 1 / eig_ratio (16 * 2^-52 / eig_ratio relative, the
    bound of the zero-covariance test below; |d e| <= e * (d2 s / 2) * that, and d2 s / 2 < 1 wherever e matters).
    Nothing is fitted to the outcome."""
    src = every_third(srcs[0.4])
    h = 1e-4
    f0, h0 = DR.score(src, cmap, T_INIT, R_frozen=T_INIT[:3, :3] if frozen else None)
    assert len(h0["i"]) > 300 and h0["faces"] == 0
    g = np.array([math.fsum(h0["terms"][:, 21 + k]) for k in range(6)])
    for k in range(6) if frozen else range(3, 6):
        D = {}
        for step in (h, 2 * h):
            xi = np.zeros(6)
            xi[k] = step
            Rf = T_INIT[:3, :3] if frozen else None
            fp, hp = DR.score(src, cmap, NR.twist_pose(xi, T_INIT), R_frozen=Rf)
            fm, hm = DR.score(src, cmap, NR.twist_pose(-xi, T_INIT), R_frozen=Rf)
            assert np.array_equal(hp["i"], h0["i"]) and np.array_equal(hp["c"], h0["c"])   # every source keeps its cells
            assert np.array_equal(hm["i"], h0["i"]) and np.array_equal(hm["c"], h0["c"])
            D[step] = (fp - fm) / (2 * step)
        trunc = abs(D[2 * h] - D[h]) / 3.0
        rounding = (12 * 2.0 ** -53 + 16 * U / EIG_RATIO) * 2 * abs(f0) / (2 * h)
        tol = 4 * trunc + rounding
        print(f"frozen {frozen} twist {k}: g {g[k]:+.9e}  -D(h) {-D[h]:+.9e}  |diff| {abs(g[k] + D[h]):.3e}  tol {tol:.3e}")
        assert abs(g[k] + D[h]) <= tol, k


# ---- 2. the Hessian --------------------------------------------------------------------------------------------------------
def test_hessian_is_symmetric_and_positive_semidefinite(cmap, srcs):
    r = DR.align(srcs[0.4], cmap, T_INIT, iters=1)
    H = full_H(r["normal"][0])
    terms = r["terms"][0]
    assert len(terms) > 500
    assert (terms[:, [0, 6, 11, 15, 18, 20]] >= 0.0).all()              # the diagonals of every per-pair block a J^T B J
    lam = np.linalg.eigvalsh(H)
    print("eigenvalues of H:", lam)
    assert lam.min() >= -1e-12 * lam.max()
    assert np.array_equal(H, H.T)


# ---- 3. the zero-covariance limit ------------------------------------------------------------------------------------------
def pair_magnitudes(q, cmap, h, d1, d2):
    """the 28 terms of every pair of an ndt_reference.hits() result with every product taken in absolute value: what a term
    is measured against where its own value is a difference of products"""
    base = np.floor(q[h["i"]] / cmap["resolution"]).astype(np.int64) + NR.OFFSETS[h["c"]]
    cell = np.searchsorted(cmap["keys"], NR.cell_key(base))
    M = np.abs(cmap["icov"][cell])
    x = np.abs(q[h["i"]] - cmap["mean"][cell])
    a = np.abs(-d1 * h["w"])
    cols = [np.abs(c) for c in LR.jacobian_columns(q[h["i"]])]
    Mv = lambda v: np.stack([NR.symrow(M, 0, v), NR.symrow(M, 1, v), NR.symrow(M, 2, v)], axis=1)
    out = [a * LR.dot3(cols[r], Mv(cols[c])) for r in range(6) for c in range(r, 6)]
    out += [a * LR.dot3(cols[r], Mv(x)) for r in range(6)]
    out.append(np.abs(-d1 * h["w"] / d2))
    return np.stack(out, axis=1)


def zero_cov_comparison(cmap, pts, T):
    d1, d2 = NR.gauss(0.55, cmap["resolution"])
    sub = pts[::40]
    q = LR.transform(sub, T)
    hp = NR.hits(q, cmap, 7, d1, d2)
    hd = DR.hits(DR.hand_sources(sub), cmap, T, 7, d1, d2)
    return hp, hd, pair_magnitudes(q, cmap, hp, d1, d2)


def test_zero_covariance_sources_give_the_point_terms(cmap, thinned):
    """Sources with C = 0 at the points themselves: B = inv3(inv3(A) + 0) is A up to the rounding of two inverses of a
    matrix of condition <= 1 / eig_ratio, 16 * 2^-52 / eig_ratio relative to the matrix, so every term agrees with the
    point path's within that, relative to the term's magnitude (its products taken in absolute value: an entry such as
    H(0, 1) is a difference of products and is not determined to that relative accuracy of ITSELF by either path;
    measured here: 2.6e-12 of itself on the worst such entry, 1.7e-13 of the magnitude; the sums agree to 1.4e-15)."""
    hp, hd, mag = zero_cov_comparison(cmap, thinned[0.4], T_INIT)
    assert len(hp["i"]) > 300
    assert np.array_equal(hp["i"], hd["i"]) and np.array_equal(hp["c"], hd["c"])
    diff = np.abs(hd["terms"] - hp["terms"])
    bound = 16 * U / EIG_RATIO
    own = diff / np.maximum(np.abs(hp["terms"]), 1e-300)
    sums = np.abs(hd["terms"].sum(0) - hp["terms"].sum(0)) / np.maximum(np.abs(hp["terms"].sum(0)), 1e-300)
    print(f"pairs {len(hp['i'])}: worst |diff| / magnitude {(diff / mag).max():.3e} (bound {bound:.3e}), / own value "
          f"{own.max():.3e}, sums {sums.max():.3e}")
    assert (diff <= bound * mag).all()
    assert sums.max() <= bound


# ---- 4. source records -----------------------------------------------------------------------------------------------------
def test_hand_built_source_cells():
    hb, names = DR.hand_built_points()
    s = DR.sources(hb, 1.0, min_points=6, eig_ratio=EIG_RATIO)
    row = {k: DR.find_source(s, v) for k, v in names.items()}
    assert s["n_src"] == (6, 2)
    assert s["count"][row["five"]] == 5 and not s["valid"][row["five"]]
    assert s["count"][row["six"]] == 6 and s["valid"][row["six"]]
    assert s["count"][row["same"]] == 6 and not s["valid"][row["same"]]
    assert (s["cov"][row["same"]] == 0.0).all()
    p = row["plane"]
    assert s["count"][p] == 6 and s["valid"][p]
    lam = np.sort(s["lam"][p])
    assert lam[0] == EIG_RATIO * lam[2] and lam[1] > lam[0]               # the flat direction is floored, exactly
    assert s["cov"][p][5] == pytest.approx(lam[0], rel=1e-12)             # and it is z
    assert list(names["neg"]) == [-1, 20, 5]                              # floor, not truncation
    assert s["count"][row["neg"]] == 1 and not s["valid"][row["neg"]] and (s["cov"][row["neg"]] == 0.0).all()
    assert list(names["face"]) == [30, 20, 5]                             # a point on a face belongs to the upper cell
    # founder order: ascending lowest point index
    assert (np.diff(s["first"]) > 0).all() and s["first"][0] == 0
    # min_points and eig_ratio are respected
    s5 = DR.sources(hb, 1.0, min_points=5, eig_ratio=0.1)
    assert s5["valid"][row["five"]] and np.sort(s5["lam"][p])[0] == 0.1 * np.sort(s5["lam"][p])[2]


def test_shuffling_the_points_reorders_the_records_and_changes_nothing_else(thinned):
    """The records depend on the order of the points inside a cell only through the order of the sums; a permutation that
    keeps every cell's points in their relative order (a stable sort by a shuffled cell rank) therefore changes the
    order of the records, to the new founder order, and not one bit of them."""
    pts = thinned[0.4][:1500]
    s = DR.sources(pts, 1.0)
    keys = NR.cell_key(NR.cell_index(pts, 1.0))
    uk = np.unique(keys)
    rank = np.random.default_rng(3).permutation(len(uk))[np.searchsorted(uk, keys)]
    perm = np.argsort(rank, kind="stable")
    t = DR.sources(pts[perm], 1.0)
    assert t["n_src"] == s["n_src"] and (np.diff(t["first"]) > 0).all()
    ks, kt = NR.cell_key(NR.cell_index(pts[s["first"]], 1.0)), NR.cell_key(NR.cell_index(pts[perm][t["first"]], 1.0))
    assert not np.array_equal(ks, kt)
    a, b = np.argsort(ks), np.argsort(kt)
    assert np.array_equal(ks[a], kt[b])
    assert DR.records(s)[a].tobytes() == DR.records(t)[b].tobytes() and np.array_equal(s["count"][a], t["count"][b])


def test_jacobi_and_eigh_routes_agree_on_the_source_covariances(srcs, thinned):
    """The map test's yardstick: the Jacobi route against numpy's eigh.  Their own spread is how far each route's
    decomposition, reassembled with nothing floored, lies from the sample covariance it decomposed; the floored
    covariances of the two routes agree within 100 x that, floored at 1e-12, relative to the cell's largest entry."""
    pts = thinned[0.2]
    sj, se = srcs[0.2], DR.sources(pts, 1.0, 6, EIG_RATIO, route="eigh")
    assert np.array_equal(sj["valid"], se["valid"]) and sj["valid"].sum() > 400
    v = sj["valid"]
    scale = np.abs(sj["scov"][v]).max(axis=1, keepdims=True)
    diff = float((np.abs(sj["cov"][v] - se["cov"][v]) / scale).max())
    spread = 0.0
    for route in ("jacobi", "eigh"):
        u = DR.sources(pts, 1.0, 6, 1e-300, route=route)                  # the same decomposition, nothing floored
        spread = max(spread, float((np.abs(u["cov"][v] - u["scov"][v]) / scale).max()))
    tol = max(100 * spread, 1e-12)
    print(f"jacobi vs eigh: {diff:.3e}; the routes' own spread {spread:.3e} -> tolerance {tol:.3e}")
    assert diff <= tol


# ---- 5. convergence and the independent check ------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf,cap_m,n_valid", [(0.2, 0.01, 483), (0.4, 0.05, 246)])
def test_the_restatement_converges_and_an_independent_d2d_agrees(cmap, srcs, leaf, cap_m, n_valid):
    src = srcs[leaf]
    assert src["n_src"][1] == n_valid
    r = DR.align(src, cmap, T_INIT, min_corr=50)
    rr = DR.align(src, cmap, T_INIT, min_corr=50, reverse=True)
    et, er = LR.pose_difference(r["pose"], T_TRUE)
    st, sr = LR.pose_difference(r["pose"], rr["pose"])
    print(f"leaf {leaf}: status {r['status']} after {r['iterations']} iterations, {r['n_corr']} sources, error {et * 1e3:.2f} mm "
          f"{er:.2e} rad; forward-vs-reversed spread {st:.2e} m {sr:.2e} rad")
    assert r["status"] == 0 and r["n_corr"] >= 50 and (r["trace"][:, 0] >= 50).all()
    assert rr["status"] == 0 and rr["iterations"] == r["iterations"]
    assert et < cap_m                                                     # a sanity cap, not a fit
    assert r["faces"] == 0 and r["boundary"] == 0
    m = DR.align_matrix(src, cmap, T_INIT, min_corr=50)
    dt, dr = LR.pose_difference(m["pose"], r["pose"])
    print(f"  independent D2D: status {m['status']} after {m['iterations']} iterations, differs by {dt:.2e} m {dr:.2e} rad")
    assert (m["status"], m["iterations"]) == (r["status"], r["iterations"])
    assert m["counts"] == [int(v) for v in r["trace"][:, 0]]
    assert dt <= max(100 * st, 1e-12) and dr <= max(100 * sr, 1e-12)


def first_valid(src, k):
    """the records of src up to its k-th valid one (the invalid ones in between keep their slots)"""
    last = np.nonzero(src["valid"])[0][k - 1] + 1
    return DR.hand_sources(src["mean"][:last], src["cov"][:last], src["valid"][:last])


@pytest.mark.parametrize("k", [31, 32, 33, 65])
def test_the_gpu_tests_one_iteration_inputs_have_no_face_and_no_boundary_case(cmap, srcs, k):
    """tests/test_hip_ndt_d2d.py compares counts exactly, which needs an input without a source on a cell face and without
    a weight on the guard's boundary: the restatement alone says so, here"""
    sub = first_valid(srcs[0.4], k)
    assert sub["n_src"][1] == k and sub["n_src"][0] > k
    r = DR.align(sub, cmap, T_INIT, iters=1, min_corr=1)
    assert (r["faces"], r["boundary"], r["status"]) == (0, 0, 1) and 0 < r["n_corr"] <= k


def test_too_few_sources_and_an_empty_map_end_with_status_2(cmap, srcs):
    src = srcs[0.4]
    r = DR.align(src, cmap, T_INIT, min_corr=src["n_src"][1] + 1)
    assert r["status"] == 2 and r["iterations"] == 1 and r["pose"].tobytes() == T_INIT.tobytes()
    r = DR.align(src, NR.cells(np.zeros((0, 3)), 1.0), T_INIT)
    assert (r["status"], r["n_corr"]) == (2, 0) and r["pose"].tobytes() == T_INIT.tobytes()


# ---- 6. argument checks and the driver -------------------------------------------------------------------------------------
def test_source_arguments_are_checked_before_any_device_work():
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser
    m = np.zeros((4, 3))
    with pytest.raises(ValueError, match="resolutions"):
        NDTLocaliser(m, source="cells", resolutions=(2.0, 1.0), device="no-such-device")
    with pytest.raises(ValueError, match="source must be"):
        NDTLocaliser(m, source="voxels", device="no-such-device")
    with pytest.raises(ValueError, match="need source='cells'"):
        NDTLocaliser(m, source_resolution=0.5, device="no-such-device")
    with pytest.raises(ValueError, match="source_resolution"):
        NDTLocaliser(m, source="cells", source_resolution=0.0, device="no-such-device")
    with pytest.raises(ValueError, match="capacity"):
        NDTLocaliser(m, source="cells", capacity=1 << 17, device="no-such-device")
    loc = object.__new__(NDTLocaliser)                                   # the refusals look at nothing but the source
    loc.source = "cells"
    rows = np.zeros((1, 4), np.float32)
    for call in (lambda: loc.submit_batch(rows, 1, np.eye(4)[None]), lambda: loc.submit_from_device(rows, 1, None),
                 lambda: loc.score_poses(rows, 1, np.eye(4)[None]), lambda: loc.relocalise(rows, 1, np.eye(4)[None])):
        with pytest.raises(ValueError, match="source='points'"):
            call()
    for kw in (dict(hypotheses=np.eye(4)[None]), dict(search=np.eye(4)[None])):
        with pytest.raises(ValueError, match="source='points'"):
            LocalisationLoop(None, loc, np.eye(4), **kw)


def test_pose_result_has_n_sources_last_with_a_default():
    import dataclasses
    from sps_amd.localiser import PoseResult
    f = dataclasses.fields(PoseResult)
    assert f[-1].name == "n_sources" and f[-1].default == 0


def test_the_binding_knows_the_d2d_entry_points():
    from sps_amd import _native
    for name in ("sps_ndt_source_scratch", "sps_ndt_source_build", "sps_ndt_align_d2d_scratch", "sps_ndt_align_d2d"):
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
    assert _native.lib.sps_version() == _native.ABI_VERSION == 202        # additive: the ABI version does not change
    assert _native.lib.sps_ndt_align_d2d_scratch(1000) == _native.lib.sps_loc_align_scratch(1000) > 0
    assert _native.lib.sps_ndt_source_scratch(1000) > 0
    assert _native.lib.sps_ndt_source_scratch(65537) == -1 and _native.lib.sps_ndt_source_scratch(-1) == -1


def test_the_drivers_list_the_source_options():
    for script in (("scripts", "filter_sequence.py"), ("tools", "localiser_timing.py")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, *script), "--help"], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-1500:]
        assert "--source" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "filter_sequence.py"), "--help"], capture_output=True,
                       text=True, cwd=ROOT)
    assert "--source-resolution" in r.stdout and "--source-min-points" in r.stdout
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "filter_sequence.py"), "--synthetic", "2", "--source", "cells"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--source needs --localise --localiser ndt" in r.stderr
