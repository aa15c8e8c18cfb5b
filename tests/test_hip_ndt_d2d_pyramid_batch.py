"""GPU tests of distribution-to-distribution NDT registered coarse to fine from several start poses
(sps_ndt_pyramid_align_d2d_batch; NDTLocaliser.submit_batch / submit_from_device / relocalise and LocalisationLoop with
d2d_pyramid=True; C ABI: the "NDT localiser, distribution to distribution, pyramid, several hypotheses" section of
include/sps_hip.h).  Device against device is bit-equal, with no tolerance: hypothesis k against
sps_ndt_pyramid_align_d2d from its pose, the final scores against sps_ndt_score_poses_d2d on a single map and single sources
of the scoring level, the map work against the point pyramid at the same pose.  The numpy restatement
(tests/ndt_d2d_pyramid_batch_reference.py) is compared within the project's rule.  The scene is
tests/test_hip_ndt_d2d_pyramid.py's (scan 1 thinned at leaf 0.4 to 4 157 points; map and sources at 2 / 1 / 0.5 m, min_corr
= 20) with the six start poses of tests/ndt_pyramid_batch_reference.py; what the tests need of these inputs is asserted from
the single calls' results."""
import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import boundary_inputs as BI
from tests import localiser_reference as LR
from tests import ndt_d2d_pyramid_batch_reference as R
from tests import ndt_d2d_pyramid_reference as DP
from tests import ndt_d2d_reference as DR
from tests import ndt_pyramid_batch_reference as PB
from tests.helpers import CFG, net_from_params, straddle_params
from tests.test_hip_ndt_d2d_pyramid import CELLS, level_capacities, make
from tests.test_ndt_cpu import KW, LEAF, T_TRUE, sensor_scan
from tests.test_ndt_d2d_cpu import first_valid

pytestmark = pytest.mark.gpu

RESOLUTIONS, MIN_CORR, POSES = R.RESOLUTIONS, R.MIN_CORR, R.POSES
FILL = 7.25            # what every output holds before a call: a row the call never wrote would keep it
STATE = 8              # NDT_PYR_STATE: done, level, slots used per level (4), and in hypothesis 0 (count of level l*, l*)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def map_xyz():
    return R.scene()["map_xyz"]


@pytest.fixture(scope="module")
def scan():
    return dev(R.scene()["scan"])


@pytest.fixture(scope="module")
def locs(map_xyz):
    """one localiser on the pyramid of source cells per setting of R.SOURCES: static, caps 30 / 30 / 30"""
    return {name: make(map_xyz, mp) for name, mp in R.SOURCES.items()}


@pytest.fixture(scope="module")
def singles(map_xyz):
    """one single-map source="cells" localiser per resolution and source_min_points: the map and the sources of a level"""
    from sps_amd.localiser import NDTLocaliser
    return {mp: [NDTLocaliser(map_xyz, resolution=r, source_min_points=mp, **CELLS) for r in RESOLUTIONS] for mp in (3, 6)}


def upload(recs, n_src=None, cap=None):
    """hand-uploaded records [L][cap][10] and n_src [L][2] (default: the rows given and the valid ones among them)"""
    recs = [np.asarray(r, dtype=np.float64).reshape(-1, 10) for r in recs]
    L = len(recs)
    cap = max(len(r) for r in recs) if cap is None else cap
    r = torch.zeros((L, max(cap, 1), 10), dtype=torch.float64, device="cuda")
    for l, rec in enumerate(recs):
        r[l, :len(rec[:cap])] = dev(rec[:cap])
    if n_src is None:
        n_src = [(len(rec), int((rec[:, 9] != 0).sum())) for rec in recs]
    return r, torch.tensor(np.asarray(n_src, dtype=np.int32).reshape(L, 2), device="cuda"), cap


@pytest.fixture(scope="module")
def device_sources(locs, scan):
    """the source cells of the scan as the device builds them, per setting of R.SOURCES: (records [3][cap][10], n_src [3][2],
    cap = the cells of the finest level), read-only.  The restatement counts the same cells."""
    out = {}
    for name, loc in locs.items():
        res = loc.submit(scan, len(scan), T_TRUE, iterations=0).result()
        assert res.n_points == len(R.scene()["pts"]) == 4157
        n = loc._n_src_lv.cpu().numpy()
        assert [tuple(int(v) for v in row) for row in n] == [s["n_src"] for s in R.scene()["src"][name]]
        cap = int(n[:, 0].max())
        out[name] = (loc._src_lv[:, :cap].contiguous().clone(), loc._n_src_lv.clone(), cap)
    return out


# ---- the C ABI itself --------------------------------------------------------------------------------------------------------
def raw_single(loc, r, n, cap, T, iters, caps, min_corr=MIN_CORR, neighbours=7):
    """sps_ndt_pyramid_align_d2d itself: every output as it lies in memory, and the state words it leaves in its scratch"""
    from sps_amd import _native
    I = max(iters, 1)
    T_out = torch.full((16,), FILL, dtype=torch.float64, device="cuda")
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    trace = torch.full((I, 4), FILL, dtype=torch.float64, device="cuda")
    normal = torch.full((I, 28), FILL, dtype=torch.float64, device="cuda")
    level = torch.full((I,), 77, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(_native.lib.sps_ndt_pyramid_align_d2d_scratch(cap), dtype=torch.uint8, device="cuda")
    loc.ctx.ndt_pyramid_align_d2d(r.data_ptr(), n.data_ptr(), cap, np.asarray(T, dtype=np.float64), iters, caps, neighbours, min_corr,
                                  loc.tol_t, loc.tol_r, T_out.data_ptr(), status.data_ptr(), trace.data_ptr() if iters else None,
                                  normal.data_ptr() if iters else None, level.data_ptr() if iters else None, scratch.data_ptr(),
                                  stream())
    loc.ctx.check_errors(stream())
    return dict(T_out=T_out.cpu().numpy(), status=status.cpu().numpy(), trace=trace.cpu().numpy()[:iters],
                normal=normal.cpu().numpy()[:iters], level=level.cpu().numpy()[:iters],
                state=scratch[-STATE * 4:].cpu().numpy().view(np.int32).copy())


def raw_batch(loc, r, n, cap, T_inits, iters, caps, min_corr=MIN_CORR, neighbours=7, scratch=None):
    """sps_ndt_pyramid_align_d2d_batch itself: every output as it lies in memory, and the state words of every hypothesis.
    T_inits: a host array [K, 4, 4] or a device tensor of K * 16 float64"""
    from sps_amd import _native
    T_dev = T_inits if torch.is_tensor(T_inits) else dev(np.asarray(T_inits, dtype=np.float64))
    K = T_dev.numel() // 16
    I = max(iters, 1)
    T_out = torch.full((K, 16), FILL, dtype=torch.float64, device="cuda")
    status = torch.full((K, 4), 77, dtype=torch.int32, device="cuda")
    trace = torch.full((K, I, 4), FILL, dtype=torch.float64, device="cuda")
    normal = torch.full((K, I, 28), FILL, dtype=torch.float64, device="cuda")
    level = torch.full((K, I), 77, dtype=torch.int32, device="cuda")
    final = torch.full((K, 2), FILL, dtype=torch.float64, device="cuda")
    best = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    T_best = torch.full((16,), FILL, dtype=torch.float64, device="cuda")
    size = _native.lib.sps_ndt_pyramid_align_d2d_batch_scratch(cap, K)
    if scratch is None:
        scratch = torch.zeros(size, dtype=torch.uint8, device="cuda")
    assert scratch.numel() >= size > 0
    loc.ctx.ndt_pyramid_align_d2d_batch(r.data_ptr(), n.data_ptr(), cap, T_dev.data_ptr(), K, iters, caps, neighbours, min_corr,
                                        loc.tol_t, loc.tol_r, T_out.data_ptr(), status.data_ptr(),
                                        trace.data_ptr() if iters else None, normal.data_ptr() if iters else None,
                                        level.data_ptr() if iters else None, final.data_ptr(), best.data_ptr(), T_best.data_ptr(),
                                        scratch.data_ptr(), stream())
    loc.ctx.check_errors(stream())
    state = scratch[size - K * STATE * 4:size].cpu().numpy().view(np.int32).reshape(K, STATE).copy()
    return dict(T_out=T_out.cpu().numpy(), status=status.cpu().numpy(), trace=trace.cpu().numpy()[:, :iters],
                normal=normal.cpu().numpy()[:, :iters], level=level.cpu().numpy()[:, :iters], final=final.cpu().numpy(),
                best=best.cpu().numpy(), T_best=T_best.cpu().numpy(), T_init=T_dev.cpu().numpy().reshape(K, 16), state=state,
                score_level=int(state[0, 7]), score_count=int(state[0, 6]))


def raw_score(one, rec, n_src, cap, poses):
    """sps_ndt_score_poses_d2d itself of a single-map localiser on one level's records: (scores [P], counts [P])"""
    from sps_amd import _native
    T_dev = dev(np.asarray(poses, dtype=np.float64).reshape(-1, 16))
    P = len(T_dev)
    out = torch.full((P, 2), FILL, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(_native.lib.sps_ndt_score_d2d_scratch(cap, P), dtype=torch.uint8, device="cuda")
    one.ctx.ndt_score_poses(rec.data_ptr(), n_src.data_ptr(), cap, T_dev.data_ptr(), P, one.neighbours, one.outlier_ratio,
                            out.data_ptr(), scratch.data_ptr(), stream(), d2d=True)
    one.ctx.check_errors(stream())
    h = out.cpu().numpy()
    return h[:, 0].copy(), h[:, 1].copy()


def assert_hypothesis_is(got, k, one, what=""):
    for name in ("T_out", "status", "trace", "normal", "level"):
        a, b = got[name][k], one[name]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, name)
    assert list(got["state"][k][:6]) == list(one["state"][:6]), (what, k, "done, level, slots used per level")


def slots_counted(levels, status):
    """the state words' slots used per level: the handoff counts a slot, so the slot that ended with status 2 or 3 is not in"""
    out = R.slots_per_level(levels)
    if status in (2, 3):
        out[int(levels[-1])] -= 1
    return out


def assert_selection(got, min_corr=MIN_CORR):
    """best and T_best follow from status, final and the poses by k_ndt_select's rule (restated in the reference module)"""
    K = len(got["status"])
    counts = got["final"][:, 1].astype(np.int64)
    b = PB.select(got["final"][:, 0], counts, got["status"][:, 0], min_corr)
    assert list(got["best"]) == PB.best_words(b, got["status"][:, 0], counts, K)
    assert got["T_best"].tobytes() == (got["T_out"][b] if b >= 0 else got["T_init"][0]).tobytes()
    return b


def assert_final_is_the_score_on(got, one, r, n, cap, level, what=""):
    """final[k] has the bits of sps_ndt_score_poses_d2d at T_out[k] on the single map of ``one`` with level ``level``'s records"""
    assert got["score_level"] == level, what
    assert got["score_count"] == int(n[level, 0].item()), what
    scores, counts = raw_score(one, r[level], n[level], cap, got["T_out"])
    assert got["final"][:, 0].tobytes() == scores.tobytes(), what
    assert got["final"][:, 1].tobytes() == counts.tobytes(), what


@pytest.fixture(scope="module")
def single_calls(locs, device_sources):
    """sps_ndt_pyramid_align_d2d of every start at every budget with all three levels live, and that the inputs are what the
    tests need"""
    r, n, cap = device_sources["all"]
    out = []
    for budget, (caps, iters) in enumerate(R.BUDGETS):
        ones = [raw_single(locs["all"], r, n, cap, T, iters, caps) for T in POSES]
        slots = [int(o["status"][1]) for o in ones]
        print(f"caps and budget {R.BUDGETS[budget]}: status {[int(o['status'][0]) for o in ones]} slots per level "
              f"{[R.slots_per_level(o['level'][:s]) for o, s in zip(ones, slots)]}")
        R.check_input_properties("all", budget, [int(o["status"][0]) for o in ones], slots,
                                 [o["level"][:s] for o, s in zip(ones, slots)])
        for o, s in zip(ones, slots):                                          # slots that did no work: zero rows and level -1
            assert not o["trace"][s:].any() and not o["normal"][s:].any() and (o["level"][s:] == -1).all()
            assert list(o["state"][2:5]) == slots_counted(o["level"][:s], o["status"][0])
        out.append(ones)
    return out


# 1. hypothesis k is the single call
@pytest.mark.parametrize("K", [1, 2, 4, 5, 64])
@pytest.mark.parametrize("budget", [0, 1, 2, 3])
def test_hypothesis_k_is_the_single_call(locs, device_sources, single_calls, budget, K):
    """caps 30 / 30 / 30, 5 / 3 / 30, 1 / 1 / 1 and a budget of 7 slots that ends in the middle of level 1"""
    r, n, cap = device_sources["all"]
    caps, iters = R.BUDGETS[budget]
    # K < 6 counts down from the start off the map, so every K has a hypothesis that is final in slot 0
    idx = [k % 6 for k in range(K)] if K == 64 else [5 - k for k in range(K)]
    got = raw_batch(locs["all"], r, n, cap, POSES[idx], iters, caps)
    for k, i in enumerate(idx):
        assert_hypothesis_is(got, k, single_calls[budget][i], (budget, K))
    assert got["T_out"][idx.index(R.OFF)].tobytes() == POSES[R.OFF].tobytes()  # status 2: the start pose, bit for bit
    b = assert_selection(got)
    assert (b == -1) == (K == 1) and got["best"][3] == K
    assert (got["score_level"], got["score_count"]) == (2, int(n[2, 0].item()))
    if K == 64:                                                                # the order changes no hypothesis' bytes
        rev = raw_batch(locs["all"], r, n, cap, POSES[idx[::-1]], iters, caps)
        for k, i in enumerate(idx[::-1]):
            assert_hypothesis_is(rev, k, single_calls[budget][i], (budget, "reversed"))
            assert rev["final"][k].tobytes() == got["final"][63 - k].tobytes()
        assert rev["final"][assert_selection(rev)].tobytes() == got["final"][b].tobytes()   # and the same score wins


# 2. the final scores
@pytest.mark.parametrize("sources", list(R.SOURCES))
def test_final_scores_are_score_poses_on_the_scoring_level(locs, singles, device_sources, scan, sources):
    """l* = 2, 1 (the finest level skipped: 3 valid sources) and 0 (nothing beyond level 0): every end pose is scored with
    level l*'s sources on level l*'s map, wherever the hypothesis stopped, bit for bit what score_poses(d2d=True) of a single
    cells localiser at that level's two resolutions and min_points gives"""
    r, n, cap = device_sources[sources]
    ls = R.CHAIN[sources][-1]
    mp = R.SOURCES[sources]
    one = singles[mp if np.ndim(mp) == 0 else mp[ls]][ls]
    for budget in (0, 3):                                                      # all end on l*; with sources on three levels none does
        caps, iters = R.BUDGETS[budget]
        got = raw_batch(locs[sources], r, n, cap, POSES, iters, caps)
        assert_final_is_the_score_on(got, one, r, n, cap, ls, (sources, budget))
        scores, counts = one.score_poses(scan, len(scan), got["T_out"].reshape(-1, 4, 4), d2d=True).result()
        assert got["final"][:, 0].tobytes() == scores.tobytes(), (sources, budget)
        np.testing.assert_array_equal(got["final"][:, 1], counts)
        assert set(got["level"][got["level"] >= 0]) <= set(R.CHAIN[sources])   # nobody enters a skipped level
        assert_selection(got)
    # iters = 0: the scores of the start poses
    got = raw_batch(locs[sources], r, n, cap, POSES, 0, (30, 30, 30))
    scores, counts = one.score_poses(scan, len(scan), POSES, d2d=True).result()
    assert got["final"][:, 0].tobytes() == scores.tobytes()
    np.testing.assert_array_equal(got["final"][:, 1], counts)
    assert got["T_out"].tobytes() == got["T_init"].tobytes() and (got["status"] == [1, 0, 0, 0]).all()
    assert counts[0] > 100 and counts[R.OFF] == 0 and got["score_level"] == ls
    assert_selection(got)


# 3. hand-made source records
@pytest.mark.parametrize("k", [31, 32, 33])
@pytest.mark.parametrize("over", [False, True])
def test_source_counts_around_a_workgroup(locs, singles, k, over):
    """every level has exactly k valid sources, k straddling the 32 sources of a workgroup of launch A (LOC_PTS).  ``over``:
    both words of n_src exceed cap_src and are clipped to it."""
    subs = [first_valid(s, k) for s in R.scene()["src"]["all"]]
    recs = [DR.records(s) for s in subs]
    cap = max(len(x) for x in recs)
    n_src = [(len(x) + (1000 if over and len(x) == cap else 0), k + (1000 if over else 0)) for x in recs]
    r, n, cap = upload(recs, n_src, cap)
    ones = [raw_single(locs["all"], r, n, cap, T, 9, (3, 3, 3)) for T in POSES]
    got = raw_batch(locs["all"], r, n, cap, POSES, 9, (3, 3, 3))
    for i, one in enumerate(ones):
        assert_hypothesis_is(got, i, one, (k, over))
    assert any(list(o["level"]) == [0] * 3 + [1] * 3 + [2] * 3 for o in ones) and got["score_level"] == 2
    scores, counts = raw_score(singles[3][2], r[2], n[2], cap, got["T_out"])
    assert got["final"][:, 0].tobytes() == scores.tobytes() and got["final"][:, 1].tobytes() == counts.tobytes()
    assert 0 < counts.max() <= k
    assert_selection(got)
    # one source fewer than min_corr everywhere: level 0 too sparse is status 2 for every hypothesis after one slot, and nobody
    # is selected
    got = raw_batch(locs["all"], r, n, cap, POSES, 9, (3, 3, 3), min_corr=k + 1 if not over else cap + 1)
    assert (got["status"][:, :2] == [2, 1]).all() and got["T_out"].tobytes() == got["T_init"].tobytes()
    assert list(got["best"]) == [-1, -1, 0, 6] and got["T_best"].tobytes() == POSES[0].tobytes() and got["score_level"] == 0


def test_a_level_with_fewer_rows_follows_one_with_more(locs, singles, device_sources):
    """level 0 with all its 443 cells (14 rows of 32 sources), then levels of 40 and 33 valid sources in 44 and 411 records (2
    and 13 rows): a partial row that level 0 left in the scratch would show in the sums of the finer levels and in the final
    pass"""
    src = R.scene()["src"]["all"]
    recs = [DR.records(src[0]), DR.records(first_valid(src[1], 40)), DR.records(first_valid(src[2], 33))]
    rows = [(len(x) + 31) // 32 for x in recs]
    assert rows[0] > rows[2] > rows[1] >= 1
    r, n, cap = upload(recs)
    caps, iters = (4, 3, 3), 10
    ones = [raw_single(locs["all"], r, n, cap, T, iters, caps) for T in POSES]
    got = raw_batch(locs["all"], r, n, cap, POSES, iters, caps)
    for i, one in enumerate(ones):
        assert_hypothesis_is(got, i, one)
    assert sum(2 in o["level"] for o in ones) >= 3                             # the input: the finest level is reached
    assert_final_is_the_score_on(got, singles[3][2], r, n, cap, 2)
    assert_selection(got)


@pytest.mark.parametrize("valid,chain", [((335, 0, 222), [0, 2]), ((335, 597, 19), [0, 1]), ((335, 19, 0), [0]),
                                         ((335, 20, 20), [0, 1, 2])])
def test_skipped_levels(locs, singles, device_sources, valid, chain):
    """the device's records with hand-set counts of valid sources: a skipped middle level, a skipped finest level, nothing
    beyond level 0, and counts that just reach min_corr"""
    r, n0, cap = device_sources["all"]
    n = n0.clone()
    n[:, 1] = torch.tensor(valid, dtype=torch.int32, device="cuda")
    caps, iters = (6, 6, 6), 18
    ones = [raw_single(locs["all"], r, n, cap, T, iters, caps) for T in POSES]
    got = raw_batch(locs["all"], r, n, cap, POSES, iters, caps)
    for i, one in enumerate(ones):
        assert_hypothesis_is(got, i, one, valid)
    live = [sorted(set(int(v) for v in o["level"] if v >= 0)) for o in ones]
    assert live[0] == chain and live[R.OFF] == [0]
    assert_final_is_the_score_on(got, singles[3][chain[-1]], r, n, cap, chain[-1], valid)
    assert assert_selection(got) not in (-1, R.OFF)


def test_level_0_too_sparse(locs, device_sources):
    r, n, cap = device_sources["all"]
    got = raw_batch(locs["all"], r, n, cap, POSES, 90, (30, 30, 30), min_corr=336)   # level 0 has 335 valid sources
    assert (got["status"][:, :2] == [2, 1]).all() and (got["status"][:, 3] == 0).all() and (got["status"][:, 2] < 336).all()
    assert got["T_out"].tobytes() == got["T_init"].tobytes()
    assert (got["level"][:, 0] == 0).all() and (got["level"][:, 1:] == -1).all()
    assert list(got["best"]) == [-1, -1, 0, 6] and got["T_best"].tobytes() == POSES[0].tobytes()
    assert got["score_level"] == 1                                            # 597 valid sources there; nobody is eligible
    ones = [raw_single(locs["all"], r, n, cap, T, 90, (30, 30, 30), min_corr=336) for T in POSES[:2]]
    for i, one in enumerate(ones):
        assert_hypothesis_is(got, i, one)


def test_status_3_from_degenerate_sources():
    """tests/test_hip_ndt_d2d_pyramid.py's input: sources whose means lie on the x axis, at the identity pose, fail the first
    pivot.  At level 0 for every hypothesis that starts there; and at level 1 behind a level 0 whose sources sit on the
    means of their map cells.  A hypothesis that starts 0.3 m to the side is not degenerate and goes on."""
    from sps_amd.localiser import NDTLocaliser
    cells = [(x, y, z) for x in range(-4, 4) for y in range(-2, 2) for z in range(-2, 2)]
    mp = BI.cell_points(cells)
    loc = NDTLocaliser(mp, resolutions=(2.0, 1.0), source_resolutions=(2.0, 1.0), min_points_per_cell=6, leaf=LEAF, source="cells",
                       min_correspondences=1)
    cov = [0.01, 0.0, 0.0, 0.01, 0.0, 0.01]
    axis = np.array([[x + 0.5, 0.0, 0.0] + cov + [1.0] for x in range(-4, 4)])
    means = loc.pyramid_cells(0)[2]
    centred = np.array([list(m) + cov + [1.0] for m in means])
    starts = np.stack([np.eye(4), LR.perturbation(0.0, 0.3, 0.1, 2.0), np.eye(4)])
    for recs, n_src, neighbours, want in (([axis, centred], [(8, 8), (16, 16)], 7, [3, 1, 8, 0]),
                                          ([centred, axis], [(16, 16), (8, 8)], 1, [3, 2, 8, 1])):
        r, n, cap = upload(recs, n_src, 16)
        ones = [raw_single(loc, r, n, cap, T, 4, (4, 4), min_corr=1, neighbours=neighbours) for T in starts]
        got = raw_batch(loc, r, n, cap, starts, 4, (4, 4), min_corr=1, neighbours=neighbours)
        for i, one in enumerate(ones):
            assert_hypothesis_is(got, i, one, want)
        assert list(got["status"][0]) == want == list(got["status"][2]) and got["T_out"][0].tobytes() == np.eye(4).tobytes()
        print(f"sources on the x axis at level {want[3]}: statuses {list(got['status'][:, 0])}, best {list(got['best'])}")
        assert got["best"][0] != 0 and got["best"][0] != 2                     # status 3 is never selected
        assert_selection(got, 1)
    loc.ctx.check_errors(stream())


def test_one_scratch_serves_64_hypotheses_and_then_two(locs, device_sources):
    from sps_amd import _native
    r, n, cap = device_sources["all"]
    caps, iters = R.BUDGETS[1]
    scratch = torch.full((_native.lib.sps_ndt_pyramid_align_d2d_batch_scratch(cap, 64),), 0xA5, dtype=torch.uint8, device="cuda")
    idx = [k % 6 for k in range(64)]
    many = raw_batch(locs["all"], r, n, cap, POSES[idx], iters, caps, scratch=scratch)
    two = raw_batch(locs["all"], r, n, cap, POSES[[R.WRONG, 2]], iters, caps, scratch=scratch)
    fresh = raw_batch(locs["all"], r, n, cap, POSES[[R.WRONG, 2]], iters, caps)
    for name in ("T_out", "status", "trace", "normal", "level", "final", "best", "T_best", "state"):
        assert two[name].tobytes() == fresh[name].tobytes(), name
    for k, i in enumerate((R.WRONG, 2)):
        for name in ("T_out", "status", "trace", "normal", "level"):
            assert two[name][k].tobytes() == many[name][i].tobytes(), (k, name)
        assert two["final"][k].tobytes() == many["final"][i].tobytes()
    assert two["best"][0] == 1 and many["best"][3] == 64


def test_arguments_are_checked(locs, singles, device_sources):
    from sps_amd import _native
    lib = _native.lib
    r, n, cap = device_sources["all"]
    loc = locs["all"]
    T_dev = dev(POSES[0])
    assert lib.sps_ndt_pyramid_align_d2d_batch_scratch(cap, 0) == lib.sps_ndt_pyramid_align_d2d_batch_scratch(cap, 65) == -1
    tail = [T_dev.data_ptr()] * 9
    for K in (0, 65):                                                          # refused before anything is launched or read
        with pytest.raises(_native.SpsError, match="n_hyp"):
            loc.ctx.ndt_pyramid_align_d2d_batch(r.data_ptr(), n.data_ptr(), cap, T_dev.data_ptr(), K, 2, (30, 30, 30), 7, 20, 1e-4, 1e-5,
                                                *tail, stream())
    for caps, neighbours in (((30, 30, 0), 7), ((30, 30, 30), 5)):             # bad level_iters; neighbours as the single call checks
        with pytest.raises(_native.SpsError):
            loc.ctx.ndt_pyramid_align_d2d_batch(r.data_ptr(), n.data_ptr(), cap, T_dev.data_ptr(), 1, 2, caps, neighbours, 20, 1e-4,
                                                1e-5, *tail, stream())
    with pytest.raises(_native.SpsError):                                      # a capacity beyond the limit
        loc.ctx.ndt_pyramid_align_d2d_batch(r.data_ptr(), n.data_ptr(), 1 << 24, T_dev.data_ptr(), 1, 2, (30, 30, 30), 7, 20, 1e-4,
                                            1e-5, *tail, stream())
    with pytest.raises(_native.SpsError, match="sps_ndt_pyramid_build has not been called"):   # the single map is no pyramid
        singles[3][0].ctx.ndt_pyramid_align_d2d_batch(r.data_ptr(), n.data_ptr(), cap, T_dev.data_ptr(), 1, 2, (30,), 7, 20, 1e-4,
                                                      1e-5, *tail, stream())
    loc.ctx.check_errors(stream())                                             # never a sticky error


# 4. against the restatement
@pytest.mark.parametrize("sources,budget", [("all", 1), ("finest skipped", 0)])
def test_the_batch_matches_the_restatement(locs, device_sources, sources, budget):
    """Statuses, slots per level, the count of every slot, l*, the sources counted on it and the selection exactly; poses and
    scores within max(100 x the restatement's own forward-versus-reversed spread on that hypothesis, 1e-12), this project's
    rule."""
    r, n, cap = device_sources[sources]
    caps, iters = R.BUDGETS[budget]
    fwd, rev = R.restated(sources, budget), R.restated(sources, budget, True)
    got = raw_batch(locs[sources], r, n, cap, POSES, iters, caps)
    misses = []
    for k, (f, b) in enumerate(zip(fwd["results"], rev["results"])):
        tol_t, tol_r, st, sr = R.spread_tolerance(f["pose"], b["pose"])
        tol_s = R.score_tolerance(fwd["scores"][k], rev["scores"][k])
        dt, dr = LR.pose_difference(got["T_out"][k].reshape(4, 4), f["pose"])
        ds = abs(got["final"][k, 0] - fwd["scores"][k])
        print(f"{R.NAMES[k]:12s}: status {got['status'][k, 0]}/{f['status']} slots {got['status'][k, 1]}/{f['iterations']} spread "
              f"{st:.3e} m {sr:.3e} rad score {abs(fwd['scores'][k] - rev['scores'][k]):.3e}; device vs restatement {dt:.3e} m "
              f"{dr:.3e} rad score {ds:.3e} (bound {tol_s:.3e})")
        assert f["faces"] == 0 and f["boundary"] == 0 and fwd["hits"][k]["faces"] == 0 and fwd["hits"][k]["boundary"] == 0
        assert list(got["status"][k]) == [f["status"], f["iterations"], f["n_corr"], f["level"]], k
        s = f["iterations"]
        np.testing.assert_array_equal(got["level"][k, :s], f["levels"])
        assert list(got["state"][k][2:5]) == slots_counted(f["levels"], f["status"]), k
        np.testing.assert_array_equal(got["trace"][k, :s, 0], f["trace"][:, 0])
        if not (dt <= tol_t and dr <= tol_r and ds <= tol_s):
            misses.append((k, dt, tol_t, dr, tol_r, ds, tol_s))
    assert not misses, misses
    assert got["score_level"] == fwd["level"] == R.CHAIN[sources][-1]
    np.testing.assert_array_equal(got["final"][:, 1], fwd["counts"])
    assert list(got["best"]) == [int(v) for v in fwd["words"]]


# 5. Python
def same_result(res, got, k):
    """PoseResult res against hypothesis k of the raw outputs"""
    code, it, n_corr, _ = (int(v) for v in got["status"][k])
    assert (res.status, res.iterations, res.n_corr) == (code, it, n_corr)
    assert res.pose.tobytes() == got["T_out"][k].tobytes() and res.trace.tobytes() == got["trace"][k, :it].tobytes()
    assert res.normal.tobytes() == got["normal"][k, :it].tobytes()
    np.testing.assert_array_equal(res.levels, got["level"][k, :it])


def same_batch_result(res, got):
    for k, x in enumerate(res.results):
        same_result(x, got, k)
    assert res.scores.tobytes() == got["final"][:, 0].tobytes()
    np.testing.assert_array_equal(res.counts, got["final"][:, 1])
    assert res.best == got["best"][0] and res.pose.tobytes() == got["T_best"].tobytes()
    assert res.score_level == got["score_level"]


@pytest.mark.parametrize("sources", ["all", "finest skipped"])
def test_submit_batch_parses_to_the_raw_call(locs, device_sources, scan, sources):
    loc = locs[sources]
    r, n, cap = device_sources[sources]
    valid = [int(v) for v in n[:, 1].cpu().numpy()]
    got = raw_batch(loc, r, n, cap, POSES, 90, (30, 30, 30))
    res = loc.submit_batch(scan, len(scan), POSES, with_normal=True, d2d_pyramid=True).result()
    assert len(res.results) == 6 and res.results[0].n_points == 4157 and res.map_update is None and res.map_carve is None
    same_batch_result(res, got)
    ls = R.CHAIN[sources][-1]
    assert (res.score_level, res.n_sources) == (ls, valid[ls])
    assert [x.n_sources for x in res.results] == [valid[ls]] * 5 + [valid[0]]  # the level of the last live slot, as submit tells
    short = loc.submit_batch(scan, len(scan), POSES[:2], iterations=4, d2d_pyramid=True).result()   # caps: (30, 30, 30)
    assert [list(x.levels) for x in short.results] == [[0, 0, 0, 0]] * 2 and short.results[0].normal is None
    assert short.score_level == ls and [x.n_sources for x in short.results] == [valid[0]] * 2
    zero = loc.submit_batch(scan, len(scan), POSES[:2], iterations=0, d2d_pyramid=True).result()
    assert [len(x.levels) for x in zero.results] == [0, 0] and zero.best == 0
    loc.ctx.check_errors(stream())


def test_submit_from_device_equals_submit(locs, scan):
    loc = locs["all"]
    src = dev(POSES[1])
    T_dev = torch.zeros(16, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        T_dev.copy_(src.reshape(-1))                                           # the kernel that writes the pose, queued in front
        pend = loc.submit_from_device(scan, len(scan), T_dev, with_normal=True, d2d_pyramid=True)
    b = pend.result()
    a = loc.submit(scan, len(scan), POSES[1], with_normal=True).result()
    x = b.results[0]
    assert b.best == 0 and a.status == 0 and len(set(a.levels)) == 3
    assert (a.status, a.iterations, a.n_corr, a.n_points, a.n_sources) == (x.status, x.iterations, x.n_corr, x.n_points, x.n_sources)
    for p, q in ((a.pose, x.pose), (a.pose, b.pose), (a.trace, x.trace), (a.normal, x.normal), (a.levels, x.levels)):
        assert p.tobytes() == q.tobytes()
    o = pend._layout()
    words = pend._host.numpy()[o["status"]:o["n_points"]].view(np.int32)
    assert list(words) == [a.status, a.iterations, a.n_corr, 2] and (b.score_level, b.n_sources) == (2, a.n_sources)


def test_relocalise_is_score_top_and_the_batch(locs, device_sources, scan):
    from sps_amd.localiser import pose_grid
    loc = locs["finest skipped"]
    r, n, cap = device_sources["finest skipped"]
    grid = POSES[1] @ pose_grid((-1.0, -0.5, 0.0, 0.5), (0.0, 0.5), (0.0, 4.0))
    P, K = len(grid), 5
    res = loc.relocalise(scan, len(scan), grid, keep=K, with_normal=True, iterations=40, d2d_pyramid=True).result()
    # by hand: the D2D scores of the single sources on the single map, the best K of them, the batch from those poses
    sp = loc.score_poses(scan, len(scan), grid, d2d=True)
    scores, counts = sp.result()
    top = torch.full((K,), -7, dtype=torch.int32, device="cuda")
    T_top = torch.zeros(K * 16, dtype=torch.float64, device="cuda")
    n_top = torch.zeros(1, dtype=torch.int32, device="cuda")
    loc.ctx.ndt_top_poses(sp._keep[2].data_ptr(), sp._keep[4].data_ptr(), P, loc.min_correspondences, K, top.data_ptr(),
                          T_top.data_ptr(), n_top.data_ptr(), stream())
    got = raw_batch(loc, r, n, cap, T_top, 40, (30, 30, 30))
    assert res.scores.tobytes() == scores.tobytes() and np.array_equal(res.counts, counts)
    np.testing.assert_array_equal(res.candidates, top.cpu().numpy())
    assert int(n_top.item()) == K and len(set(res.candidates)) == K
    same_batch_result(res.batch, got)
    assert res.index == res.candidates[res.batch.best] and res.ok and res.pose.tobytes() == got["T_best"].tobytes()
    assert res.batch.score_level == 1 and res.batch.n_sources == 246
    loc.ctx.check_errors(stream())


def test_a_frame_queued_behind_a_filter(locs, map_xyz):
    from sps_amd.sps_filters import SPSFilter
    loc = locs["all"]
    params = straddle_params(O.random_params(seed=0), synthetic.small_scene(seed=11, n_scan=2500))
    net = net_from_params(params).cuda().eval().freeze()
    f = SPSFilter(net, map_xyz.astype(np.float32), voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=CFG["FILTER"]["THRESHOLD"])
    pend = f.submit(sensor_scan(4), T_TRUE)
    starts = POSES[[1, R.OFF, 2]]
    a = loc.submit_filtered_batch(pend, starts, with_normal=True, d2d_pyramid=True).result()   # before the frame's result()
    fres = pend.result()
    assert 0 < len(fres.filtered) <= 12800
    b = loc.submit_batch(fres.filtered.clone(), len(fres.filtered), starts, with_normal=True, d2d_pyramid=True).result()
    assert a.best == b.best and a.best in (0, 2) and a.pose.tobytes() == b.pose.tobytes() and a.score_level == b.score_level
    assert a.scores.tobytes() == b.scores.tobytes() and a.counts.tobytes() == b.counts.tobytes()
    for x, y in zip(a.results, b.results):
        assert (x.status, x.iterations, x.n_corr, x.n_points, x.n_sources) == (y.status, y.iterations, y.n_corr, y.n_points, y.n_sources)
        assert x.pose.tobytes() == y.pose.tobytes() and x.trace.tobytes() == y.trace.tobytes() and x.normal.tobytes() == y.normal.tobytes()
    assert a.results[0].iterations > 3 and a.results[1].status == 2


CARVE = dict(min_pass=1, miss_frames=1)        # one frame clears: the carve leaves a trace in the maps


def test_the_online_pyramid_is_updated_and_carved_as_the_point_pyramid_s_batch_leaves_it(map_xyz, locs, scan):
    """submit_batch(d2d_pyramid=True, integrate=True, carve=True) on an online pyramid with source cells: the registration has
    the static pyramid's bits, and every level ends as the point pyramid's level ends when its batch selects the same pose"""
    from sps_amd.localiser import NDTLocaliser
    caps = level_capacities(map_xyz)
    online = make(map_xyz, level_capacities=caps)
    points = NDTLocaliser(map_xyz, resolutions=RESOLUTIONS, leaf=LEAF, level_capacities=caps)
    starts = POSES[[R.OFF, R.WRONG, 2]]
    plain = locs["all"].submit_batch(scan, len(scan), starts, with_normal=True, d2d_pyramid=True).result()
    got = online.submit_batch(scan, len(scan), starts, with_normal=True, d2d_pyramid=True, integrate=True, carve=True,
                              carve_options=CARVE).result()
    assert got.best == plain.best == 2 and got.pose.tobytes() == plain.pose.tobytes() and got.scores.tobytes() == plain.scores.tobytes()
    assert isinstance(got.map_update, tuple) and len(got.map_update) == 3 and isinstance(got.map_carve, tuple) and len(got.map_carve) == 3
    # the point pyramid's batch of no iterations from that pose selects it and works on the map there
    twin = points.submit_batch(scan, len(scan), got.pose[None], iterations=0, coarse_to_fine=True, integrate=True, carve=True,
                               carve_options=CARVE).result()
    assert twin.best == 0 and twin.pose.tobytes() == got.pose.tobytes()
    assert got.map_update == twin.map_update and got.map_carve == twin.map_carve
    assert all(u.points > 0 for u in got.map_update) and all(c.rays > 0 for c in got.map_carve)
    for l in range(3):
        for a, b in zip(online.pyramid_cells(l), points.pyramid_cells(l)):
            assert a.tobytes() == b.tobytes(), l
        for a, b in zip(online.carve_state(l), points.carve_state(l)):
            assert a.tobytes() == b.tobytes(), l
        assert online.pyramid_info(l) == points.pyramid_info(l)
    # nobody selected: no byte of any level moves
    before = [[a.tobytes() for a in online.pyramid_cells(l)] for l in range(3)]
    off = POSES[[R.OFF] * 2]
    res = online.submit_batch(scan, len(scan), off, d2d_pyramid=True, integrate=True, carve=True, carve_options=CARVE).result()
    assert res.best == -1 and res.pose.tobytes() == off[0].tobytes()
    assert [(u.founded, u.dropped, u.points) for u in res.map_update] == [(0, 0, 0)] * 3
    assert [(c.rays, c.seen_through, c.cleared, c.cut) for c in res.map_carve] == [(0, 0, 0, 0)] * 3
    assert before == [[a.tobytes() for a in online.pyramid_cells(l)] for l in range(3)]
    with pytest.raises(ValueError):                                            # a static pyramid has no map to integrate into
        locs["all"].submit_batch(scan, len(scan), starts, d2d_pyramid=True, integrate=True)
    online.ctx.check_errors(stream())


class RestatementOnDevice:
    """tests/ndt_d2d_pyramid_reference.py behind the interface LocalisationLoop uses on the host path, with a real PendingPose
    whose device buffer the estimator's correction reads"""
    source = "cells"

    def __init__(self, cmaps, like):
        self.cmaps, self.like, self.device = cmaps, like, like.device
        self.resolutions, self.source_resolutions = like.resolutions, like.source_resolutions
        self.tolerances = []                                                   # per frame: R.spread_tolerance of its alignment

    def submit_filtered(self, pending, T_init):
        from sps_amd.localiser import PendingPose, _pose_layout
        count = int(pending.count_dev.item())
        rows = pending._filtered[:count].cpu().numpy()
        L = self.like
        pts = LR.downsample(rows, count, L.leaf, L.capacity)[1]
        S = DP.sources(pts, L.source_resolutions, L.source_level_min_points, L.eig_ratio)
        x = DP.align(S, self.cmaps, T_init, L.iterations, L.level_iterations, L.neighbours, L.min_correspondences,
                     L.outlier_ratio, L.tol_t, L.tol_r)
        assert x["faces"] == 0 and x["boundary"] == 0
        rev = DP.align(S, self.cmaps, T_init, L.iterations, L.level_iterations, L.neighbours, L.min_correspondences,
                       L.outlier_ratio, L.tol_t, L.tol_r, reverse=True)
        self.tolerances.append(R.spread_tolerance(x["pose"], rev["pose"]))
        K, n_lv = x["iterations"], len(S)
        o = _pose_layout(K, False, True, None, False, False, False, n_lv)
        h = np.zeros(o["total"])
        h[o["T_out"]:o["status"]] = x["pose"].ravel()
        h[o["status"]:o["n_points"]].view(np.int32)[:] = [x["status"], K, x["n_corr"], x["level"]]
        h[o["n_points"]:o["trace"]].view(np.int32)[:] = [len(pts), 0]
        h[o["trace"]:o["normal"]] = x["trace"].ravel()
        h[o["sources"]:o["levels"]].view(np.int32)[:n_lv] = [DP.valid_sources(s) for s in S]
        h[o["levels"]:o["update"]].view(np.int32)[:K] = x["levels"]
        out = dev(h)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return PendingPose(K, False, torch.from_numpy(h.copy()), ev, (None, None, out, None, None), True, None, False, False, False,
                           n_lv)


def test_three_loop_frames_on_the_device_path_follow_the_restatement():
    """LocalisationLoop(SPSCVMFilter, the cells pyramid, ukf, d2d_pyramid=True) on the estimator's device path over three frames
    of the synthetic sequence at epsilon = 2 (every point passes), against the same loop driven by the restatement from the
    host: status, slots, levels, counts and sources of every frame.  Frame 0 starts from the same pose on both sides, so its
    pose and the estimator's pose after its correction are held to max(100 x the restatement's forward-versus-reversed
    spread on that frame, 1e-12); the later frames start from the poses before them, and their differences are printed."""
    import math

    from sps_amd.localiser import LocalisationLoop
    from sps_amd.pose_estimator import PoseEstimator
    from sps_amd.sps_filters import SPSCVMFilter
    frames, step = 3, 0.5
    mp = synthetic.sequence_map(frames, step, **KW)
    truth, scans = [], []
    for i in range(frames):
        world = synthetic.lidar_scan(100 + i, x_offset=step * i, **KW)
        T = LR.perturbation(step * i, 0.0, 0.0, math.degrees(0.02 * i))
        Ti = np.linalg.inv(T)
        scans.append(np.c_[world[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3], world[:, 3]].astype(np.float32))
        truth.append(T)
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(np.ascontiguousarray(mp[:, :3], dtype=np.float32))
    map64 = mp[:, :3].astype(np.float64)

    def run(localiser, **kw):
        est = PoseEstimator(truth[0], "cuda", initial_velocity=(step / 0.1, 0.0, 0.0))
        loop = LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0), localiser, truth[0],
                                estimator=est, **kw)
        return loop, [loop.step(s, dt=0.1) for s in scans]

    ndt = make(map64)
    loop, steps = run(ndt, d2d_pyramid=True)
    ref = RestatementOnDevice(DP.pyramid(map64, RESOLUTIONS), ndt)
    ref_loop, ref_steps = run(ref)
    assert loop.device_guess is True and ref_loop.device_guess is False and len(ref.tolerances) == frames
    for i, (s, t) in enumerate(zip(steps, ref_steps)):
        a, b = s.pose_result, t.pose_result
        dt, dr = LR.pose_difference(loop.poses[i], ref_loop.poses[i])
        et, er = LR.pose_difference(s.estimate, t.estimate)
        print(f"frame {i}: status {a.status}/{b.status} slots {a.iterations}/{b.iterations} levels "
              f"{np.bincount(a.levels, minlength=3)}/{np.bincount(b.levels, minlength=3)} count {a.n_corr}/{b.n_corr} sources "
              f"{a.n_sources}/{b.n_sources}; device vs restatement {dt:.3e} m {dr:.3e} rad, estimates {et:.3e} m {er:.3e} rad")
        assert (a.status, a.iterations, a.n_corr, a.n_points, a.n_sources) == (b.status, b.iterations, b.n_corr, b.n_points,
                                                                               b.n_sources), i
        np.testing.assert_array_equal(a.levels, b.levels)
        assert not s.flagged and not t.flagged and s.batch is not None and len(s.batch.results) == 1 and t.batch is None, i
        if i == 0:
            tol_t, tol_r = ref.tolerances[0][:2]
            assert s.guess.tobytes() == t.guess.tobytes()
            assert dt <= tol_t and dr <= tol_r and et <= tol_t and er <= tol_r, (dt, dr, et, er, tol_t, tol_r)
        assert a.status in (0, 1) and s.batch.score_level == a.levels[-1] == 2 and len(set(a.levels)) == 3, i
    ndt.ctx.check_errors(stream())


def test_the_loop_takes_hypotheses_and_search_on_an_online_pyramid(map_xyz, scan):
    from sps_amd.localiser import LocalisationLoop, pose_grid
    online = make(map_xyz, caps=(10, 10, 10), level_capacities=level_capacities(map_xyz))

    class Kept:
        """a filter that takes no pose and keeps every row, its rows on the device"""
        takes_pose = False

        def submit(self, rows):
            res = type("Result", (), dict(filtered=rows))()
            return type("Pending", (), dict(_filtered=rows, count_dev=torch.full((1,), len(rows), dtype=torch.int32, device="cuda"),
                                            result=lambda self: res))()
    loop = LocalisationLoop(Kept(), online, POSES[1], hypotheses=pose_grid((0.0, 0.5), (0.0,), (0.0,)),
                            search=pose_grid((0.0, 0.5, -0.5), (0.0,), (0.0, 4.0)), search_keep=3, update_map=True, carve_map=True,
                            d2d_pyramid=True)
    first, second = loop.step(scan), loop.step(scan)
    assert first.search is not None and first.search.ok and second.search is None and second.batch is not None
    for st, K in ((first, 3), (second, 2)):
        b = st.batch
        assert not st.flagged and b.best >= 0 and len(b.results) == K and b.score_level == 2 and b.n_sources == 222
        assert isinstance(b.map_update, tuple) and len(b.map_update) == 3 and all(u.points > 0 for u in b.map_update)
        assert isinstance(b.map_carve, tuple) and len(b.map_carve) == 3 and all(c.rays > 0 for c in b.map_carve)
        assert LR.pose_difference(st.pose, T_TRUE)[0] < 0.05
    online.ctx.check_errors(stream())


# 6. unchanged behaviour, bit for bit
def test_the_other_calls_give_the_bits_they_gave_before(map_xyz, locs, singles, scan):
    """submit_batch(d2d=True) on the single map, plain submit on the pyramid of source cells and
    submit_batch(coarse_to_fine=True) on a point pyramid: the same bytes before and after calls with d2d_pyramid=True on the
    same localiser, which are those of localisers that never saw one; and the refusals stay"""
    from sps_amd.localiser import NDTLocaliser
    loc = make(map_xyz, 6)                                                     # never saw the new keyword
    seen = locs["finest skipped"]
    poses = np.stack([LR.perturbation(o, 0.0, 0.0, 0.0) @ T_TRUE for o in (0.0, 0.2, 0.5)])

    def look(x):
        b = x.submit_batch(scan, len(scan), poses, with_normal=True, iterations=5, d2d=True)
        s = x.submit(scan, len(scan), poses[2], with_normal=True)
        rb, rs = b.result(), s.result()
        return b._host.numpy().tobytes(), s._host.numpy().tobytes(), [v.n_sources for v in rb.results], rs.n_sources, rb.score_level

    before = look(loc)
    res = loc.submit_batch(scan, len(scan), poses, d2d_pyramid=True).result()
    assert res.best >= 0 and res.score_level == 1
    assert look(loc) == before == look(seen)
    assert before[2:] == ([246] * 3, 246, None)
    plain = singles[6][1].submit_batch(scan, len(scan), poses, with_normal=True, iterations=5, d2d=True)
    plain.result()
    assert plain._host.numpy().tobytes() == before[0]                          # ... and of a localiser without a pyramid
    one = NDTLocaliser(map_xyz, resolutions=RESOLUTIONS, leaf=LEAF, iterations=12, level_iterations=(4, 4, 4))
    a = one.submit_batch(scan, len(scan), poses, with_normal=True, coarse_to_fine=True)
    b = one.submit_batch(scan, len(scan), poses, with_normal=True, coarse_to_fine=True, d2d_pyramid=False)
    ra, rb = a.result(), b.result()
    assert a._host.numpy().tobytes() == b._host.numpy().tobytes() and ra.score_level is None and ra.n_sources is None
    assert ra.best >= 0 and len(set(ra.results[0].levels)) == 3
    T_dev = dev(poses[0])
    for call in (lambda **kw: loc.submit_batch(scan, len(scan), poses, **kw), lambda **kw: loc.relocalise(scan, len(scan), poses, **kw),
                 lambda **kw: loc.submit_from_device(scan, len(scan), T_dev, **kw)):
        with pytest.raises(ValueError, match="d2d=True and coarse_to_fine exclude each other"):
            call(d2d=True, coarse_to_fine=True)
        with pytest.raises(ValueError, match="source='points'"):
            call()
        with pytest.raises(ValueError, match="d2d_pyramid=True excludes"):
            call(d2d_pyramid=True, d2d=True)
    for x in (one, singles[6][1]):
        with pytest.raises(ValueError, match="d2d_pyramid=True needs"):
            x.submit_batch(scan, len(scan), poses, d2d_pyramid=True)
    loc.ctx.check_errors(stream())
