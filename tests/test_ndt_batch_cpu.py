"""CPU tests of the NDT localiser with several hypotheses: pose_grid, the selection rule, and the restatement
(tests/ndt_batch_reference.py) on the 18-hypothesis scene the GPU test re-uses.  No GPU."""
import functools

import numpy as np
import pytest

from tests import localiser_reference as LR
from tests import ndt_batch_reference as NB
from tests import ndt_reference as NR
from tests.test_ndt_cpu import KW, LEAF, T_INIT, T_TRUE, sensor_scan

ALONG, ACROSS, YAW = (-1.5, 0.0, 1.5), (-1.0, 0.0, 1.0), (0.0, 8.0)
CENTRE = (1 * len(ACROSS) + 1) * len(YAW) + 0              # a = 0, b = 0, psi = 0


@functools.lru_cache(maxsize=1)
def scene18():
    """The scene of tests/test_hip_ndt.py (map with the hand-built cells, scan 1 thinned at LEAF) registered by the
    restatement from the 18 start poses T_INIT @ D(a, b, psi).  Computed once per process, shared with the GPU test, never
    modified."""
    from sps_amd import synthetic
    hb, _ = NR.hand_built_cells()
    map_xyz = np.concatenate([synthetic.build_map(**KW)[:, :3].astype(np.float64), hb])
    cmap = NR.cells(map_xyz, 1.0)
    scan = sensor_scan(1)
    _, pts = LR.downsample(scan, len(scan), LEAF)
    starts = np.stack([T_INIT @ d for d in NB.grid(ALONG, ACROSS, YAW)])
    return dict(map_xyz=map_xyz, cmap=cmap, scan=scan, pts=pts, starts=starts, ref=NB.align_batch(pts, cmap, starts))


def test_pose_grid_order_and_identity():
    from sps_amd.localiser import pose_grid
    g = pose_grid(ALONG, ACROSS, YAW)
    assert g.shape == (18, 4, 4) and g.dtype == np.float64
    k = 0
    for a in ALONG:
        for b in ACROSS:
            for y in YAW:
                np.testing.assert_array_equal(g[k], NB.offset(a, b, y))
                k += 1
    assert g[CENTRE].tobytes() == np.eye(4).tobytes()                       # the identity, in its place, exactly
    assert g[CENTRE + 1][0, 1] == -np.sin(np.radians(8.0)) and g[0][0, 3] == -1.5 and g[0][1, 3] == -1.0
    assert (g[:, 2, :] == [0.0, 0.0, 1.0, 0.0]).all() and (g[:, 3, :] == [0.0, 0.0, 0.0, 1.0]).all()
    one = pose_grid(0.0, 0.0, 0.0)
    assert one.shape == (1, 4, 4) and np.array_equal(one[0], np.eye(4))


def test_the_loop_checks_its_hypotheses():
    from sps_amd.localiser import LocalisationLoop, pose_grid

    class Batch:
        device = "cpu"

        def submit_batch(self, *a):
            raise AssertionError

    g = pose_grid(ALONG, ACROSS, YAW)
    with pytest.raises(ValueError):
        LocalisationLoop(None, Batch(), np.eye(4), hypotheses=g)           # the identity is not at index 0
    with pytest.raises(ValueError):
        LocalisationLoop(None, Batch(), np.eye(4), hypotheses=np.tile(np.eye(4), (65, 1, 1)))
    with pytest.raises(TypeError):
        LocalisationLoop(None, object(), np.eye(4), hypotheses=g[[CENTRE]])  # a localiser without submit_batch
    front = np.concatenate([g[[CENTRE]], np.delete(g, CENTRE, axis=0)])
    loop = LocalisationLoop(None, Batch(), np.eye(4), hypotheses=front)
    assert loop.start_poses(T_INIT)[0].tobytes() == (T_INIT @ np.eye(4)).tobytes()
    assert LocalisationLoop(None, object(), np.eye(4)).hypotheses is None   # today's loop


def test_selection_rule():
    sel = NB.select
    assert sel([1.0, 3.0, 2.0], [100, 100, 100], [0, 0, 0], 50) == 1
    assert sel([3.0, 3.0, 2.0], [100, 100, 100], [0, 1, 0], 50) == 0        # a tie goes to the lowest index
    assert sel([1.0, 3.0, 3.0], [100, 100, 100], [0, 1, 0], 50) == 1
    assert sel([1.0, 3.0, 2.0], [100, 100, 100], [0, 2, 1], 50) == 2        # status 2 is out whatever its score
    assert sel([1.0, 3.0, 2.0], [100, 100, 100], [0, 3, 1], 50) == 2        # so is status 3
    assert sel([1.0, 3.0, 2.0], [100, 49, 50], [0, 0, 0], 50) == 2          # too few points counted at the final pose
    assert sel([1.0, 3.0, 2.0], [10, 10, 10], [0, 0, 0], 50) == -1
    assert sel([1.0, 3.0], [100, 100], [2, 3], 50) == -1
    assert sel([0.0], [50], [1], 50) == 0                                   # a score of 0 still qualifies


def test_the_restatement_selects_the_centre_hypothesis():
    s = scene18()
    ref = s["ref"]
    scores, best = ref["scores"], ref["best"]
    for k, r in enumerate(ref["results"]):
        et, er = LR.pose_difference(r["pose"], T_TRUE)
        print(f"hypothesis {k:2d}: status {r['status']} iterations {r['iterations']:2d} score {scores[k]:10.2f} "
              f"count {ref['counts'][k]} error {et:.4f} m {er:.5f} rad")
    assert len(s["pts"]) > 4000 and len(scores) == 18
    assert best == CENTRE
    assert s["starts"][CENTRE].tobytes() == (T_INIT @ np.eye(4)).tobytes()
    # its end pose is the single alignment's, and so is its error
    single = NR.align(s["pts"], s["cmap"], T_INIT @ np.eye(4))
    assert ref["results"][best]["pose"].tobytes() == single["pose"].tobytes() == ref["pose"].tobytes()
    et, _ = LR.pose_difference(ref["pose"], T_TRUE)
    assert et < 0.02
    # a condition on the input: the winner leads the runner-up by more than 1e-6 of its score, so the order in which a
    # score's ~10^4 terms are added (relative effect <= 1e-12) cannot change the selection
    runner = np.sort(scores)[-2]
    print(f"best {scores[best]:.2f}, runner-up {runner:.2f}, margin {scores[best] - runner:.3f}")
    assert scores[best] - runner > 1e-6 * scores[best]
    # the confident failures the batch exists for: a start 1.5 m along converges (status 0) far from the true pose
    wrong = [k for k, r in enumerate(ref["results"]) if r["status"] == 0 and LR.pose_difference(r["pose"], T_TRUE)[0] > 0.5]
    assert wrong and all(scores[k] < scores[best] for k in wrong)


def test_the_binding_knows_the_batch_entry_points():
    from sps_amd import _native
    for name in ("sps_ndt_align_batch_scratch", "sps_ndt_align_batch"):
        assert name in _native.EXPORTS and hasattr(_native.lib, name)
    assert _native.lib.sps_version() == _native.ABI_VERSION                 # additive: the ABI version does not change
    one, many = _native.lib.sps_ndt_align_batch_scratch(1000, 1), _native.lib.sps_ndt_align_batch_scratch(1000, 64)
    assert one >= _native.lib.sps_ndt_align_scratch(1000) - 16 and many >= 64 * (one - 16)
    for cap, k in ((-1, 1), (1000, 0), (1000, 65)):
        assert _native.lib.sps_ndt_align_batch_scratch(cap, k) == -1
