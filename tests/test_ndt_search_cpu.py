"""CPU tests of the NDT pose search: the restatement (tests/ndt_search_reference.py) against ndt_batch_reference, the
top-K rule on hand-made tables, and the 75-pose grid the GPU test re-uses, with the two conditions that make its outcome
well defined.  No GPU."""
import functools
import math

import numpy as np
import pytest

from tests import localiser_reference as LR
from tests import ndt_batch_reference as NB
from tests import ndt_reference as NR
from tests import ndt_search_reference as NS
from tests.test_ndt_batch_cpu import scene18
from tests.test_ndt_cpu import T_TRUE

# 5 along x 3 across x 5 yaw = 75 poses (two pose tiles of 32 and a rest of 11) around a centre 1.2 m and 6 degrees off
ALONG, ACROSS, YAW = (-2.0, -1.0, 0.0, 1.0, 2.0), (-0.5, 0.0, 0.5), (-10.0, -5.0, 0.0, 5.0, 10.0)
T_CENTRE = T_TRUE @ NB.offset(1.1, -0.4, 6.0)
KEEP = 8
MIN_CORR = 50


@functools.lru_cache(maxsize=1)
def search75():
    """scene18()'s map and thinned scan, the 75 poses T_CENTRE @ D_k, their scores in the restatement and the
    restatement's relocalise.  Computed once per process, shared with the GPU test, never modified."""
    s = scene18()
    poses = np.stack([T_CENTRE @ d for d in NB.grid(ALONG, ACROSS, YAW)])
    grid = NS.score_poses(s["pts"], s["cmap"], poses)
    return dict(map_xyz=s["map_xyz"], cmap=s["cmap"], scan=s["scan"], pts=s["pts"], poses=poses, grid=grid,
                ref=NS.relocalise(s["pts"], s["cmap"], poses, KEEP, scores=grid))


def test_score_equals_a_batch_of_zero_iterations():
    s = search75()
    some = [0, 26, 37, 74]
    b = NB.align_batch(s["pts"], s["cmap"], s["poses"][some], iters=0)
    for j, k in enumerate(some):
        assert b["results"][j]["pose"].tobytes() == s["poses"][k].tobytes() and b["results"][j]["iterations"] == 0
        assert np.float64(b["scores"][j]).tobytes() == np.float64(s["grid"]["scores"][k]).tobytes(), k
        assert b["counts"][j] == s["grid"]["counts"][k], k
        # the kernels' order of summation stays within the bound the GPU test grants the device
        bound = NS.sum_bound(s["grid"]["m"][k], len(s["pts"]), s["grid"]["sum_abs"][k])
        assert abs(s["grid"]["ordered"][k] - s["grid"]["scores"][k]) <= bound, k
    assert (s["grid"]["ordered"] != s["grid"]["scores"]).any()            # and it is another order


def test_ordered_sum_is_the_stated_order():
    rng = np.random.default_rng(3)
    n = 32 * 19 + 5                                                         # 20 blocks: runs of 3, the last run short
    i = np.repeat(np.arange(n), 2)
    c = np.tile([0, 3], n)
    v = rng.random(2 * n) * 10.0 ** rng.integers(-8, 8, 2 * n)
    per_point = v[0::2] + v[1::2]
    part = []
    for b in range(20):
        acc = 0.0
        for x in per_point[32 * b:32 * b + 32]:
            acc = acc + x
        part.append(acc)
    runs = []
    for sg in range(8):
        acc = 0.0
        for x in part[3 * sg:3 * sg + 3]:
            acc = acc + x
        runs.append(acc)
    want = 0.0
    for x in runs:
        want = want + x
    assert NS.ordered_sum(i, c, v, n) == want
    assert NS.ordered_sum(i[:0], c[:0], v[:0], 0) == 0.0


def test_top_rule():
    top = NS.top
    idx, n = top([1.0, 3.0, 2.0, 5.0], [100] * 4, 50, 2)
    assert idx.tolist() == [3, 1] and n == 2
    idx, n = top([3.0, 1.0, 3.0, 3.0], [100] * 4, 50, 3)                    # ties keep the lowest index first
    assert idx.tolist() == [0, 2, 3] and n == 3
    idx, n = top([3.0, float("nan"), 2.0, float("nan")], [100] * 4, 50, 4)  # NaN never qualifies
    assert idx.tolist() == [0, 2, -1, -1] and n == 2
    idx, n = top([9.0, 3.0, 2.0], [49, 50, 51], 50, 3)                      # counts below min_corr are out whatever the score
    assert idx.tolist() == [1, 2, -1] and n == 2
    idx, n = top([1.0, 2.0], [100, 100], 50, 5)                             # K larger than the number of qualifiers
    assert idx.tolist() == [1, 0, -1, -1, -1] and n == 2
    idx, n = top([1.0, 2.0], [10, 10], 50, 3)                               # nobody qualifies
    assert idx.tolist() == [-1, -1, -1] and n == 0
    idx, n = top([0.0, 0.0], [0, 0], 0, 1)                                  # min_corr = 0: a score of 0 qualifies
    assert idx.tolist() == [0] and n == 1
    poses = np.arange(3)[:, None, None] * np.ones((3, 4, 4))
    assert NS.top_poses(poses, np.array([2, 1, -1, -1]))[:, 0, 0].tolist() == [2.0, 1.0, 2.0, 2.0]   # the fill rule
    assert NS.top_poses(poses, np.array([-1, -1]))[:, 0, 0].tolist() == [0.0, 0.0]


def test_the_grid_is_well_defined_and_ends_in_the_true_basin():
    s = search75()
    g, ref = s["grid"], s["ref"]
    P, n = len(s["poses"]), len(s["pts"])
    assert P == 75 and P > 64 and P % 32 != 0 and n > 4000 and g["faces"].sum() == 0
    order = NS.top(g["scores"], g["counts"], MIN_CORR, P)[0]
    assert (order >= 0).all()
    for r in range(KEEP + 2):
        k = order[r]
        et, er = LR.pose_difference(s["poses"][k], T_TRUE)
        print(f"rank {r}: pose {k} score {g['scores'][k]:.3f} count {g['counts'][k]} bound "
              f"{NS.sum_bound(g['m'][k], n, g['sum_abs'][k]):.3e} off by {et:.3f} m {er:.4f} rad")
    # condition 1: the order of the first KEEP + 1 poses, and with it the candidate set, cannot change with the order in
    # which a score's terms are added: neighbours in the ranking differ by more than both their summation bounds
    for r in range(KEEP):
        a, b = order[r], order[r + 1]
        gap = g["scores"][a] - g["scores"][b]
        assert gap > NS.sum_bound(g["m"][a], n, g["sum_abs"][a]) + NS.sum_bound(g["m"][b], n, g["sum_abs"][b]), r
    assert ref["candidates"].tolist() == order[:KEEP].tolist() and ref["n_top"] == KEEP
    # condition 2: the best pose of the grid lies in the true basin, and relocalise ends where test_ndt_batch_cpu.py
    # accepts its centre hypothesis
    top1 = NR.align(s["pts"], s["cmap"], s["poses"][order[0]])
    assert top1["status"] == 0 and LR.pose_difference(top1["pose"], T_TRUE)[0] < 0.02
    et, er = LR.pose_difference(ref["pose"], T_TRUE)
    print(f"relocalise: index {ref['index']} best {ref['batch']['best']} statuses {[r['status'] for r in ref['batch']['results']]} "
          f"final scores {ref['batch']['scores']} error {et:.4f} m {er:.5f} rad")
    assert ref["index"] >= 0 and ref["index"] == ref["candidates"][ref["batch"]["best"]] and et < 0.02
    # the centre of the grid is no such start: a single alignment from it ends in another basin, which is why one searches
    centre = NR.align(s["pts"], s["cmap"], T_CENTRE)
    assert LR.pose_difference(centre["pose"], T_TRUE)[0] > 0.5
    # a condition on the input: several candidates end in the true basin, a few 1e-5 apart in score (they stop within the
    # alignment's tolerances of one another); the winner leads the runner-up by more than 100 x the two summation bounds,
    # the factor the pose tolerance of the GPU tests grants the device's end poses
    b = ref["batch"]
    fs = np.argsort(-b["scores"], kind="stable")
    bounds = [NS.sum_bound(len(b["hits"][k]["terms"]), n, math.fsum(np.abs(b["hits"][k]["terms"][:, 27]))) for k in fs[:2]]
    print(f"final scores: best {b['scores'][fs[0]]!r} runner-up {b['scores'][fs[1]]!r} bounds {bounds}")
    assert fs[0] == b["best"] and b["scores"][fs[0]] - b["scores"][fs[1]] > 100.0 * sum(bounds)


def test_the_loop_checks_its_search():
    from sps_amd.localiser import LocalisationLoop, pose_grid

    class Search:
        device = "cpu"

        def relocalise(self, *a, **k):
            raise AssertionError

    g = pose_grid(ALONG, ACROSS, YAW)
    centre = (2 * len(ACROSS) + 1) * len(YAW) + 2
    assert g[centre].tobytes() == np.eye(4).tobytes()
    front = np.concatenate([g[[centre]], np.delete(g, centre, axis=0)])
    with pytest.raises(ValueError):
        LocalisationLoop(None, Search(), np.eye(4), search=g)               # the identity is not at index 0
    with pytest.raises(ValueError):
        LocalisationLoop(None, Search(), np.eye(4), search=np.eye(4))       # not [P, 4, 4]
    with pytest.raises(ValueError):
        LocalisationLoop(None, Search(), np.eye(4), search=front, search_keep=65)
    with pytest.raises(TypeError):
        LocalisationLoop(None, object(), np.eye(4), search=front)           # a localiser without relocalise
    loop = LocalisationLoop(None, Search(), np.eye(4), search=front)
    assert loop.search_poses(T_TRUE)[0].tobytes() == (T_TRUE @ np.eye(4)).tobytes() and len(loop.search_poses(T_TRUE)) == 75
    assert LocalisationLoop(None, object(), np.eye(4)).search is None       # today's loop


def test_the_binding_knows_the_search_entry_points():
    from sps_amd import _native
    from sps_amd.localiser import MAX_POSES
    for name in ("sps_ndt_score_scratch", "sps_ndt_score_poses", "sps_ndt_top_poses"):
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
    assert _native.lib.sps_version() == _native.ABI_VERSION
    sc = _native.lib.sps_ndt_score_scratch
    assert MAX_POSES == 65536
    assert sc(1000, 1) == 32 * 16 and sc(1000, 75) == 75 * 32 * 16 and sc(0, 3) == 3 * 16
    assert sc(1 << 16, 65536) <= 64 << 20 and sc(1 << 16, 65536) % (32 * 2048 * 16) == 0   # chunks of whole tiles
    assert sc(1 << 23, 65536) == 32 * (1 << 18) * 16                        # one tile of poses where that alone is more
    for cap, p in ((-1, 1), (1000, 0), (1000, 65537), ((1 << 23) + 1, 1)):
        assert sc(cap, p) == -1
