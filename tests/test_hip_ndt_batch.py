"""GPU tests of the NDT localiser with several hypotheses (sps_amd.localiser.NDTLocaliser.submit_batch; C ABI: the "NDT
localiser, several hypotheses" section of include/sps_hip.h) against single alignments and against the numpy restatement
in tests/ndt_batch_reference.py.  Shapes are those of test_hip_ndt.py: 400 x 32 rays, ~4.2 k points after thinning."""
import math

import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_batch_reference as NB
from tests import ndt_reference as NR
from tests.helpers import CFG, net_from_params, straddle_params
from tests.test_ndt_batch_cpu import CENTRE, scene18
from tests.test_ndt_cpu import KW, LEAF, T_INIT, T_TRUE, sensor_scan

pytestmark = pytest.mark.gpu

RES = 1.0
TOL_FLOOR = 1e-12      # this project's rule for float64 comparisons that differ only in the order of a sum


@pytest.fixture(scope="module")
def scene():
    return scene18()


@pytest.fixture(scope="module")
def loc(scene):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF)


@pytest.fixture(scope="module")
def loc1(scene):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(scene["map_xyz"], resolution=RES, leaf=LEAF, neighbours=1)


@pytest.fixture(scope="module")
def batch18(loc, scene):
    """the 18-hypothesis batch on the device, computed once"""
    scan = dev(scene["scan"])
    return loc.submit_batch(scan, len(scan), scene["starts"], with_normal=True).result()


@pytest.fixture(scope="module")
def tol(scene):
    """the pose tolerance of test_hip_ndt.py: 100 x the restatement's forward / reversed spread, floored at 1e-12"""
    fwd = scene["ref"]["results"][CENTRE]
    rev = NR.align(scene["pts"], scene["cmap"], scene["starts"][CENTRE], reverse=True)
    spread_t, spread_r = LR.pose_difference(fwd["pose"], rev["pose"])
    t = max(100.0 * spread_t, TOL_FLOOR), max(100.0 * spread_r, TOL_FLOOR)
    print(f"spread forward/reversed: {spread_t:.3e} m {spread_r:.3e} rad -> tolerance {t[0]:.3e} m {t[1]:.3e} rad")
    return t


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    assert (a.status, a.iterations, a.n_corr, a.n_points) == (b.status, b.iterations, b.n_corr, b.n_points)
    for x, y in ((a.pose, b.pose), (a.trace, b.trace), (a.normal, b.normal)):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()


def same_batch(a, b):
    assert len(a.results) == len(b.results) and a.best == b.best
    for x, y in zip(a.results, b.results):
        same_bits(x, y)
    assert a.scores.tobytes() == b.scores.tobytes() and a.counts.tobytes() == b.counts.tobytes()
    assert a.pose.tobytes() == b.pose.tobytes()


# ---- a batch is K single alignments ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("neighbours,n_hyp", [(7, 18), (1, 18), (7, 1)])
def test_batch_equals_single_calls(loc, loc1, scene, neighbours, n_hyp):
    L = loc if neighbours == 7 else loc1
    scan = dev(scene["scan"])
    starts = scene["starts"][:n_hyp] if n_hyp > 1 else scene["starts"][[CENTRE]]
    got = L.submit_batch(scan, len(scan), starts, with_normal=True).result()
    assert len(got.results) == n_hyp and got.scores.shape == (n_hyp,) and got.counts.shape == (n_hyp,)
    ran = set()
    for k in range(n_hyp):
        one = L.submit(scan, len(scan), starts[k], with_normal=True).result()
        same_bits(got.results[k], one)
        assert got.results[k].normal is not None and one.iterations >= 1
        ran.add((one.status, one.iterations))
    assert n_hyp == 1 or len(ran) > 1          # the hypotheses did not all take the same course
    assert got.pose.tobytes() == (got.results[got.best].pose if got.best >= 0 else starts[0]).tobytes()
    L.ctx.check_errors(stream())


# ---- against the restatement -----------------------------------------------------------------------------------------------
def test_batch_matches_the_restatement(batch18, scene, tol):
    """Final scores: the device adds the m per-cell scores of a pose in its fixed order, the restatement with math.fsum;
    the bound (m + 6) * 2^-52 * sum |term| is that of test_hip_ndt.py::test_one_iteration_matches_the_restatement."""
    ref = scene["ref"]
    assert len(batch18.results) == 18
    for k, (a, b) in enumerate(zip(batch18.results, ref["results"])):
        dt, dr = LR.pose_difference(a.pose, b["pose"])
        terms = ref["hits"][k]["terms"][:, 27]
        bound = (len(terms) + 6) * 2.0 ** -52 * math.fsum(np.abs(terms))
        print(f"hypothesis {k:2d}: status {a.status}/{b['status']} iterations {a.iterations}/{b['iterations']} count "
              f"{a.n_corr}/{b['n_corr']} final count {batch18.counts[k]}/{ref['counts'][k]} pose {dt:.3e} m {dr:.3e} rad "
              f"score {batch18.scores[k]!r} / {ref['scores'][k]!r} |diff| {abs(batch18.scores[k] - ref['scores'][k]):.3e} "
              f"bound {bound:.3e}")
    for k, (a, b) in enumerate(zip(batch18.results, ref["results"])):
        assert b["faces"] == 0 and b["boundary"] == 0 and ref["hits"][k]["faces"] == 0, k   # exact counts need such an input
        assert (a.status, a.iterations, a.n_corr) == (b["status"], b["iterations"], b["n_corr"]), k
        np.testing.assert_array_equal(a.trace[:, 0], b["trace"][:, 0])
        assert batch18.counts[k] == ref["counts"][k], k
        dt, dr = LR.pose_difference(a.pose, b["pose"])
        assert dt <= tol[0] and dr <= tol[1], k
        terms = ref["hits"][k]["terms"][:, 27]
        assert abs(batch18.scores[k] - ref["scores"][k]) <= (len(terms) + 6) * 2.0 ** -52 * math.fsum(np.abs(terms)), k
    assert batch18.best == ref["best"] == CENTRE
    assert batch18.pose.tobytes() == batch18.results[batch18.best].pose.tobytes()
    et, _ = LR.pose_difference(batch18.pose, T_TRUE)
    rt, _ = LR.pose_difference(ref["pose"], T_TRUE)
    assert et <= rt + tol[0]


def test_two_batches_give_the_same_bits(loc, scene, batch18):
    scan = dev(scene["scan"])
    same_batch(batch18, loc.submit_batch(scan, len(scan), scene["starts"], with_normal=True).result())


# ---- edges -----------------------------------------------------------------------------------------------------------------
def test_a_hypothesis_off_the_map_leaves_its_neighbours_alone(loc, scene, batch18):
    scan = dev(scene["scan"])
    starts = scene["starts"].copy()
    starts[3, 0, 3] += 500.0
    got = loc.submit_batch(scan, len(scan), starts, with_normal=True).result()
    r = got.results[3]
    assert r.status == 2 and r.iterations == 1 and r.n_corr < loc.min_correspondences
    assert r.pose.tobytes() == starts[3].tobytes()                          # the start pose, bit for bit
    assert got.counts[3] < loc.min_correspondences
    for k in range(18):
        if k != 3:
            same_bits(got.results[k], batch18.results[k])
            assert got.scores[k] == batch18.scores[k] and got.counts[k] == batch18.counts[k]
    assert got.best == batch18.best and got.pose.tobytes() == batch18.pose.tobytes()
    loc.ctx.check_errors(stream())


def test_no_hypothesis_qualifies(loc, scene):
    scan = dev(scene["scan"])
    starts = scene["starts"][:5].copy()
    starts[:, 0, 3] += 500.0
    got = loc.submit_batch(scan, len(scan), starts).result()
    assert got.best == -1 and [r.status for r in got.results] == [2] * 5
    assert got.pose.tobytes() == starts[0].tobytes()
    assert all(r.pose.tobytes() == s.tobytes() for r, s in zip(got.results, starts))
    loc.ctx.check_errors(stream())                                          # never a sticky error
    none = loc.submit_batch(scan, 0, scene["starts"][:3]).result()          # count = 0
    assert none.best == -1 and [(r.status, r.n_points) for r in none.results] == [(2, 0)] * 3
    assert (none.scores == 0.0).all() and (none.counts == 0).all() and none.pose.tobytes() == scene["starts"][0].tobytes()
    empty_rows = loc.submit_batch(torch.zeros((0, 4), dtype=torch.float32, device="cuda"), 0, scene["starts"][:2]).result()
    assert empty_rows.best == -1 and empty_rows.pose.tobytes() == scene["starts"][0].tobytes()
    loc.ctx.check_errors(stream())


def test_an_empty_map(scene):
    from sps_amd.localiser import NDTLocaliser
    empty = NDTLocaliser(np.zeros((0, 3)), resolution=RES, leaf=LEAF)
    got = empty.submit_batch(dev(scene["scan"]), len(scene["scan"]), scene["starts"][:4]).result()
    assert got.best == -1 and got.pose.tobytes() == scene["starts"][0].tobytes()
    assert [(r.status, r.iterations, r.n_corr, r.n_points) for r in got.results] == [(2, 1, 0, len(scene["pts"]))] * 4
    assert (got.scores == 0.0).all() and (got.counts == 0).all()
    empty.ctx.check_errors(stream())


def test_duplicate_hypotheses_tie_to_the_lower_index(loc, scene, batch18):
    scan = dev(scene["scan"])
    s = scene["starts"]
    got = loc.submit_batch(scan, len(scan), np.stack([s[0], s[CENTRE], s[CENTRE], s[10]]), with_normal=True).result()
    same_bits(got.results[1], got.results[2])
    same_bits(got.results[1], batch18.results[CENTRE])
    assert got.scores[1] == got.scores[2] == batch18.scores[CENTRE] and got.scores[1] > got.scores[3] > got.scores[0]
    assert got.best == 1


def test_arguments_are_checked(loc, scene):
    from sps_amd import _native
    scan = dev(scene["scan"])
    for bad in (np.zeros((0, 4, 4)), np.tile(np.eye(4), (65, 1, 1)), np.eye(4), np.full((2, 4, 4), np.nan)):
        with pytest.raises(ValueError):
            loc.submit_batch(scan, len(scan), bad)
    with pytest.raises(TypeError):
        loc.submit_batch(torch.zeros((4, 4)), 4, scene["starts"][:2])       # a host tensor
    # the C entry point itself
    n = torch.tensor([100], dtype=torch.int32, device="cuda")
    pts = torch.zeros((128, 3), dtype=torch.float64, device="cuda")
    T = dev(np.tile(np.eye(4), (65, 1, 1)))
    out = torch.zeros(65 * 16 + 65 * 2 + 65 * 2 * 4 + 65 * 2 + 2 + 16, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(_native.lib.sps_ndt_align_batch_scratch(128, 64), dtype=torch.uint8, device="cuda")
    p = out.data_ptr()
    o_status, o_trace, o_final, o_best, o_Tb = p + 65 * 16 * 8, p + 65 * 18 * 8, p + 65 * 26 * 8, p + 65 * 28 * 8, p + (65 * 28 + 2) * 8

    def call(T_ptr, n_hyp):
        loc.ctx.ndt_align_batch(pts.data_ptr(), n.data_ptr(), 128, T_ptr, n_hyp, 2, 7, 50, 0.55, 1e-4, 1e-5, p, o_status, o_trace,
                                None, o_final, o_best, o_Tb, scratch.data_ptr(), stream())

    for T_ptr, n_hyp in ((T.data_ptr(), 0), (T.data_ptr(), 65), (None, 4)):
        with pytest.raises(_native.SpsError) as e:
            call(T_ptr, n_hyp)
        assert e.value.code == _native.ERR_INVALID
    call(T.data_ptr(), 64)                                                  # the largest batch is accepted
    torch.cuda.synchronize()
    best = out[65 * 28:65 * 28 + 2].cpu().numpy().view(np.int32)
    assert -1 <= best[0] < 64 and best[3] == 64
    loc.ctx.check_errors(stream())


# ---- stream order: the filter's pending frame goes straight in -------------------------------------------------------------
def test_submit_filtered_batch_equals_result_then_submit_batch(loc, scene):
    from sps_amd.sps_filters import SPSFilter
    params = straddle_params(O.random_params(seed=0), synthetic.small_scene(seed=11, n_scan=2500))
    net = net_from_params(params).cuda().eval().freeze()
    f = SPSFilter(net, scene["map_xyz"].astype(np.float32), voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=CFG["FILTER"]["THRESHOLD"])
    scan = sensor_scan(4)
    starts = scene["starts"][[CENTRE, 10, 12, 3]]
    pend = f.submit(scan, T_TRUE)
    pose_pend = loc.submit_filtered_batch(pend, starts, with_normal=True)   # before the frame's result()
    a = pose_pend.result()
    fres = pend.result()
    assert 0 < len(fres.filtered) <= len(scan)
    b = loc.submit_batch(fres.filtered.clone(), len(fres.filtered), starts, with_normal=True).result()
    same_batch(a, b)


# ---- the closed loop -------------------------------------------------------------------------------------------------------
def test_closed_loop_with_hypotheses_follows_the_restatement(tol):
    """LocalisationLoop(SPSCVMFilter, NDTLocaliser, hypotheses) over the 8 synthetic frames of test_hip_ndt.py's loop test,
    with two hypotheses: the guess, and the guess moved one 0.5 m step along the direction of travel (the lag the loop
    without hypotheses never recovers).  The filter runs at epsilon = 2 (every point passes)."""
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser, pose_grid
    from sps_amd.sps_filters import SPSCVMFilter
    from sps_amd.trajectory import ape_translation
    n, step = 8, 0.5
    mp = synthetic.sequence_map(n, step, **KW)
    truth, scans = [], []
    for i in range(n):
        world = synthetic.lidar_scan(100 + i, x_offset=step * i, **KW)
        T = LR.perturbation(step * i, 0.0, 0.0, math.degrees(0.02 * i))
        Ti = np.linalg.inv(T)
        scans.append(np.c_[world[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3], world[:, 3]].astype(np.float32))
        truth.append(T)
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(np.ascontiguousarray(mp[:, :3], dtype=np.float32))
    map64 = mp[:, :3].astype(np.float64)
    hyp = pose_grid((0.0, step), 0.0, 0.0)
    assert np.array_equal(hyp[0], np.eye(4))

    def run(localiser, **kw):
        loop = LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0), localiser, truth[0], **kw)
        steps = [loop.step(s) for s in scans]
        return loop.poses, steps

    ndt = NDTLocaliser(map64, resolution=RES, leaf=LEAF)
    got, steps = run(ndt, hypotheses=hyp)
    want, ref_steps = run(NB.BatchLocaliser(NR.cells(map64, RES), ndt), hypotheses=hyp)
    plain, plain_steps = run(ndt)
    print("APE with hypotheses:", ape_translation(got, truth), " without:", ape_translation(plain, truth))
    for i in range(n):
        a, b = steps[i].batch, ref_steps[i].batch
        dt, dr = LR.pose_difference(got[i], want[i])
        print(f"frame {i}: best {a.best}/{b.best} status {[r.status for r in a.results]}/{[r.status for r in b.results]} "
              f"iterations {[r.iterations for r in a.results]}/{[r.iterations for r in b.results]} scores {a.scores} / {b.scores} "
              f"device vs restatement {dt:.3e} m {dr:.3e} rad")
    for i in range(n):
        a, b = steps[i].batch, ref_steps[i].batch
        assert a.best == b.best and steps[i].flagged == ref_steps[i].flagged == (a.best < 0), i
        assert [r.status for r in a.results] == [r.status for r in b.results], i
        assert steps[i].pose_result is a.results[max(a.best, 0)]
        dt, dr = LR.pose_difference(got[i], want[i])
        assert dt <= tol[0] and dr <= tol[1], i
    # hypotheses = None is the loop as it was: no batch, and the poses of a loop given the argument's default
    again, again_steps = run(ndt, hypotheses=None)
    assert all(s.batch is None for s in plain_steps + again_steps)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(plain, again))
    for s, t in zip(plain_steps, again_steps):
        same_bits(s.pose_result, t.pose_result)
    # and one identity hypothesis registers exactly what the loop without hypotheses registers
    single, single_steps = run(ndt, hypotheses=np.eye(4)[None])
    for i, (s, t) in enumerate(zip(plain_steps, single_steps)):
        assert t.batch.best == (-1 if s.flagged else 0), i
        assert (s.pose_result.status, s.pose_result.iterations, s.pose_result.n_corr) == \
               (t.pose_result.status, t.pose_result.iterations, t.pose_result.n_corr), i
        assert plain[i].tobytes() == single[i].tobytes(), i
    ndt.ctx.check_errors(stream())
