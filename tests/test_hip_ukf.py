"""The device pose estimator (include/sps_hip.h, "pose estimator") against its restatement tests/ukf_reference.py, bit for
bit, and around the NDT localiser: submit_from_device, frames queued without a host synchronisation, the loop."""
import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import localiser_reference as LR
from tests import ndt_reference as NR
from tests import ukf_reference as UR
from tests.helpers import CFG, net_from_params
from tests.test_ndt_cpu import KW, LEAF, T_INIT, T_TRUE, sensor_scan

pytestmark = pytest.mark.gpu

RES = 1.0
TOL_FLOOR = 1e-12
T0 = LR.perturbation(1.0, -2.0, 0.5, 25.0)
V0 = (2.0, 0.5, -0.1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def estimator(T=T0, v=V0, **kw):
    from sps_amd.pose_estimator import PoseEstimator
    return PoseEstimator(T, "cuda", initial_velocity=v, **kw)


def imu_rows(m, seed=0):
    rng = np.random.default_rng(seed)
    rows = np.zeros((m, 7))
    rows[:, 0] = 0.01
    rows[:, 1:4] = rng.normal(0.0, 1.0, (m, 3)) + [0.0, 0.0, 9.81]
    rows[:, 4:7] = rng.normal(0.0, 0.3, (m, 3)) + [0.05, -0.02, 0.5]
    return rows


def assert_state(est, ref, what=""):
    s = est.state()
    for name, a, b in (("mean", s.mean, ref.x), ("covariance", s.covariance, ref.P), ("pose", s.pose, ref.T)):
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)
            raise AssertionError(f"{what} {name}: {len(bad)} entries differ, first {bad[0]}: {a[tuple(bad[0])]!r} != "
                                 f"{b[tuple(bad[0])]!r} (max |diff| {np.abs(a - b).max():.3e})")
    assert (s.n_predict, s.n_correct) == (ref.predicts, ref.corrects), what
    return s


# ---- the kernels against the restatement -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def warmed():
    """a reference state with a full covariance: two predictions and a correction from the start"""
    ref = UR.init(T0, V0)
    UR.predict(ref, imu_rows(2, seed=9))
    UR.correct(ref, LR.perturbation(1.05, -1.98, 0.5, 26.0))
    return ref


def warm(est):
    est.predict_imu(imu_rows(2, seed=9))
    est.correct(LR.perturbation(1.05, -1.98, 0.5, 26.0))


def test_init_matches_the_restatement():
    for T in (T0, np.eye(4), LR.perturbation(0, 0, 0, 179.0), np.diag([1.0, -1.0, -1.0, 1.0]), np.diag([-1.0, 1.0, -1.0, 1.0])):
        est = estimator(T)
        s = assert_state(est, UR.init(T, V0), "init")
        assert est.pose_dev.cpu().numpy().tobytes() == s.pose.tobytes() and s.predict_samples == 0


@pytest.mark.parametrize("m", [0, 1, 2, 5, 256])
def test_predict_imu_is_bit_equal_to_the_restatement(m, warmed):
    est = estimator()
    warm(est)
    ref = warmed.copy()
    rows = imu_rows(m, seed=m)
    est.predict_imu(rows)
    info = UR.predict(ref, rows)
    s = assert_state(est, ref, f"M = {m}")
    assert [s.predict_status, s.predict_samples, s.predict_failed] == list(info[:3]) == [0, m, -1]
    assert est.pose_dev.cpu().numpy().tobytes() == ref.T.tobytes()
    assert s.covariance.tobytes() == np.ascontiguousarray(s.covariance.T).tobytes()
    if m:
        assert s.mean.tobytes() != warmed.x.tobytes()


def test_predict_dt_is_bit_equal_to_the_restatement(warmed):
    est = estimator()
    warm(est)
    ref = warmed.copy()
    for dt in (0.1, 0.037):
        est.predict(dt)
        assert list(UR.predict_dt(ref, dt)) == [0, 1, -1, 0]
        assert_state(est, ref, f"dt = {dt}")
    assert est.pose_dev.cpu().numpy().tobytes() == ref.T.tobytes()


@pytest.mark.parametrize("gate", [None, 0, 1, 2, 3, -1])
def test_correct_is_bit_equal_to_the_restatement(gate, warmed):
    est = estimator()
    warm(est)
    est.predict(0.1)
    ref = warmed.copy()
    UR.predict_dt(ref, 0.1)
    before = est.state_dev.clone()
    Tm = LR.perturbation(1.3, -1.9, 0.52, 27.0)
    want_status, want_nu = UR.correct(ref, Tm, gate=gate)
    if gate is None:
        est.correct(Tm)
    else:
        Td, words = dev(Tm), torch.tensor([7, gate], dtype=torch.int32, device="cuda")     # the gate is the second word
        est._correct(Td.data_ptr(), words.data_ptr() + 4)
    s = assert_state(est, ref, f"gate {gate}")
    assert s.status == want_status == (0 if gate in (None, 0, 1) else 2)
    assert s.innovation.tobytes() == want_nu.tobytes()
    closed = gate not in (None, 0, 1)
    assert torch.equal(before, est.state_dev) == closed                # a closed gate: every byte of the state block
    assert bool(s.innovation.any()) != closed


def test_a_measurement_on_the_other_side_of_the_sphere_is_negated():
    """yaw -91 degrees (Shepperd's R22 branch: z > 0) against a state at yaw -89 (the trace branch: w > 0, z < 0): the two
    quaternions have a negative dot product"""
    Ta, Tb = LR.perturbation(0, 0, 0, -89.0), LR.perturbation(0.1, 0, 0, -91.0)
    qa, qb = UR.measurement_of(Ta)[3:], UR.measurement_of(Tb)[3:]
    assert float(qa @ qb) < -0.5
    est, ref = estimator(Ta), UR.init(Ta, V0)
    est.predict(0.1)
    UR.predict_dt(ref, 0.1)
    est.correct(Tb)
    status, nu = UR.correct(ref, Tb)
    s = assert_state(est, ref, "-q")
    assert status == s.status == 0 and s.innovation.tobytes() == nu.tobytes() and np.abs(nu[3:]).max() < 0.5
    z = UR.measurement_of(Tb)
    z[3:] = -z[3:]
    other = UR.init(Ta, V0)
    UR.predict_dt(other, 0.1)
    UR.correct_z(other, z)
    assert other.x.tobytes() == ref.x.tobytes() and other.P.tobytes() == ref.P.tobytes()


def test_a_singular_covariance_is_status_3_and_leaves_the_state_alone():
    est, ref = estimator(initial_cov=0.0), UR.init(T0, V0, 0.0)
    before = est.state_dev.clone()
    est.predict(0.1)
    s = est.state()
    assert [s.predict_status, s.predict_samples, s.predict_failed] == list(UR.predict_dt(ref, 0.1)[:3]) == [3, 0, 0]
    est.correct(T0)
    s = assert_state(est, ref, "singular")
    assert s.status == UR.correct(ref, T0)[0] == 3 and not s.innovation.any()
    assert torch.equal(before, est.state_dev)
    assert est.pose_dev.cpu().numpy().tobytes() == ref.T.tobytes()        # the pose handed on is the state's


def test_a_failing_sample_leaves_the_state_of_the_sample_before_it(warmed):
    """through the C ABI, past the Python check that refuses such rows: sample 3 of 6 is not finite"""
    from sps_amd import _native
    est = estimator()
    warm(est)
    ref = warmed.copy()
    rows = imu_rows(6, seed=4)
    rows[3, 5] = np.nan
    d = dev(rows)
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    _native.check(_native.lib.sps_ukf_predict(est._state_ptr, d.data_ptr(), 6, est._Q, est._pred_ptr, info.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
    want = UR.predict(ref, rows)
    assert info.cpu().tolist() == list(want) == [3, 3, 3, 0]
    assert_state(est, ref, "failing sample")
    rows[0, 0] = -0.01                                                   # and a dt that is not > 0, at sample 0: nothing moves
    d = dev(rows)
    _native.check(_native.lib.sps_ukf_predict(est._state_ptr, d.data_ptr(), 6, est._Q, est._pred_ptr, info.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
    assert info.cpu().tolist() == list(UR.predict(ref, rows)) == [3, 0, 0, 0]
    assert_state(est, ref, "failing first sample")


def test_two_calls_give_the_same_bits():
    out = []
    for _ in range(2):
        est = estimator()
        est.predict_imu(imu_rows(40, seed=2))
        est.correct(LR.perturbation(1.8, -1.6, 0.46, 31.0))
        est.predict(0.05)
        out.append(est.state_dev.cpu().numpy().tobytes())
    assert out[0] == out[1]


# ---- around the localiser ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def map_xyz():
    return synthetic.build_map(**KW)[:, :3].astype(np.float64)


@pytest.fixture(scope="module")
def cmap(map_xyz):
    return NR.cells(map_xyz, RES)


@pytest.fixture(scope="module")
def loc(map_xyz):
    from sps_amd.localiser import NDTLocaliser
    return NDTLocaliser(map_xyz, resolution=RES, leaf=LEAF)


@pytest.fixture(scope="module")
def tolerance(cmap):
    """the pose tolerance of tests/test_hip_ndt.py::test_full_alignment_matches_the_restatement: 100 x the restatement's
    forward-against-reversed spread on scan 1, floored at 1e-12"""
    scan = sensor_scan(1)
    _, pts = LR.downsample(scan, len(scan), LEAF)
    fwd, rev = NR.align(pts, cmap, T_INIT), NR.align(pts, cmap, T_INIT, reverse=True)
    st, sr = LR.pose_difference(fwd["pose"], rev["pose"])
    return max(100.0 * st, TOL_FLOOR), max(100.0 * sr, TOL_FLOOR)


def test_submit_from_device_equals_submit(loc, map_xyz):
    assert len(map_xyz) > 50000
    for seed, T in ((1, T_INIT), (2, T_TRUE)):
        scan = dev(sensor_scan(seed))
        assert len(scan) > 10000
        a = loc.submit(scan, len(scan), T, with_normal=True).result()
        b = loc.submit_from_device(scan, len(scan), dev(T), with_normal=True).result()
        r = b.results[0]
        assert b.best == 0 and (a.status, a.iterations, a.n_corr, a.n_points) == (r.status, r.iterations, r.n_corr, r.n_points)
        assert a.iterations > 1 and a.status == 0
        assert a.pose.tobytes() == r.pose.tobytes() == b.pose.tobytes()
        assert a.trace.tobytes() == r.trace.tobytes() and a.normal.tobytes() == r.normal.tobytes()
    with pytest.raises(TypeError):
        loc.submit_from_device(scan, len(scan), T_INIT)
    with pytest.raises(TypeError):
        loc.submit_from_device(scan, len(scan), dev(T_INIT.astype(np.float32)))


def test_three_frames_queued_without_a_host_synchronisation(loc, cmap, tolerance):
    """predict -> submit_from_device -> correct_from, three times on a side stream, then one wait"""
    tol_t, tol_r = tolerance
    scans = [sensor_scan(s) for s in (1, 2, 3)]
    dscans = [dev(s) for s in scans]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        est = estimator(T_INIT, (0.0, 0.0, 0.0))
        pend = []
        for d in dscans:
            est.predict(0.1)
            pend.append(loc.submit_from_device(d, len(d), est.pose_dev))
            est.correct_from(pend[-1])
        wait = est.snapshot()
    state, _ = wait()                                                      # the one wait
    got = [p.result() for p in pend]
    # the restatement-driven chain
    chain = UR.init(T_INIT)
    replay = UR.init(T_INIT)                                               # ... and the restatement fed the device's own poses
    for k, (scan, b) in enumerate(zip(scans, got)):
        UR.predict_dt(chain, 0.1)
        _, pts = LR.downsample(scan, len(scan), LEAF)
        r = NR.align(pts, cmap, chain.T)
        UR.correct(chain, r["pose"], gate=r["status"])
        a = b.results[0]
        dt, dr = LR.pose_difference(a.pose, r["pose"])
        print(f"frame {k}: status {a.status}/{r['status']} iterations {a.iterations}/{r['iterations']} device vs restatement "
              f"{dt:.3e} m {dr:.3e} rad (tolerance {tol_t:.3e} {tol_r:.3e})")
        assert (a.status, a.iterations, a.n_points) == (r["status"], r["iterations"], len(pts)) and a.status == 0
        assert dt <= tol_t and dr <= tol_r
        UR.predict_dt(replay, 0.1)
        gate = a.status if b.best == 0 else -1
        assert UR.correct(replay, b.pose, gate=gate)[0] == 0
    for name, a, b in (("mean", state.mean, replay.x), ("covariance", state.covariance, replay.P), ("pose", state.pose, replay.T)):
        assert a.tobytes() == b.tobytes(), name
    assert (state.n_predict, state.n_correct, state.status) == (3, 3, 0)
    et, _ = LR.pose_difference(state.pose, T_TRUE)
    assert et < 0.1                                                        # and the filter ended near the truth, from 0.3 m off


class RawFilter:
    """every point passes: what LocalisationLoop needs of a filter that takes no pose and keeps its rows on the device"""
    takes_pose = False

    def submit(self, scan):
        rows = scan if torch.is_tensor(scan) else torch.from_numpy(np.ascontiguousarray(scan, dtype=np.float32)).cuda()
        count = torch.full((1,), len(rows), dtype=torch.int32, device="cuda")

        class Pending:
            _filtered, count_dev = rows, count

            def result(self):
                class Result:
                    filtered = rows
                return Result()
        return Pending()


def test_an_empty_scan_flags_the_frame_and_leaves_the_estimator_alone(loc):
    from sps_amd.localiser import LocalisationLoop
    est = estimator(T_INIT, (0.0, 0.0, 0.0))
    loop = LocalisationLoop(RawFilter(), loc, T_INIT, estimator=est)
    assert loop.device_guess is True
    a = loop.step(sensor_scan(1))
    assert not a.flagged and a.pose_result.status == 0 and a.guess.tobytes() == T_INIT.tobytes()
    before = est.state_dev.clone()
    b = loop.step(np.zeros((0, 4), np.float32), dt=0.1)
    predicted = est.state_dev.clone()
    assert b.flagged and b.pose_result.status == 2 and b.batch.best == -1
    assert b.pose.tobytes() == b.guess.tobytes() == b.estimate.tobytes()     # the guess is handed on
    ref = est.state()
    assert ref.status == 2 and ref.n_correct == 1 and ref.n_predict == 1 and not torch.equal(before, predicted)
    # bit-identical to an estimator that made the same prediction and was never offered the frame
    twin = estimator(T_INIT, (0.0, 0.0, 0.0))
    twin.predict_imu(np.zeros((0, 7)))
    twin.correct_from(loc.submit_from_device(dev(sensor_scan(1)), len(sensor_scan(1)), twin.pose_dev))
    twin.predict(0.1)
    assert torch.equal(twin.state_dev, est.state_dev)
    c = loop.step(sensor_scan(2), dt=0.1)
    assert not c.flagged and LR.pose_difference(c.estimate, T_TRUE)[0] < 0.1


def test_without_an_estimator_the_loop_is_todays(loc):
    from sps_amd.localiser import FEW_CORRESPONDENCES, SINGULAR, LocalisationLoop
    from sps_amd.sps_filters import ConstantVelocityModel
    scans = [sensor_scan(s) for s in (1, 2, 3, 4, 5, 6)]
    loop = LocalisationLoop(RawFilter(), loc, T_INIT)
    steps = [loop.step(s) for s in scans]
    model = ConstantVelocityModel()
    model.poses = []
    for k, (scan, st) in enumerate(zip(scans, steps)):
        guess = model.predict() if len(model.poses) >= 4 else model.poses[-1].copy() if model.poses else T_INIT.copy()
        r = loc.submit(dev(scan), len(scan), guess).result()
        flagged = r.status in (FEW_CORRESPONDENCES, SINGULAR)
        pose = guess if flagged else r.pose
        model.add_pose(pose)
        assert st.guess.tobytes() == guess.tobytes() and st.pose.tobytes() == pose.tobytes() and st.flagged == flagged, k
        p = st.pose_result
        assert (p.status, p.iterations, p.n_corr, p.n_points) == (r.status, r.iterations, r.n_corr, r.n_points)
        assert p.pose.tobytes() == r.pose.tobytes() and p.trace.tobytes() == r.trace.tobytes()
        assert st.batch is None and st.search is None and st.estimate is None
        assert st.filter_result.filtered.shape == (len(scan), 4)
    assert len(loop.poses) == 6 and loop.estimator is None and loop.device_guess is False


@pytest.fixture(scope="module")
def sequence():
    """the synthetic sequence of the driver's --synthetic 8 replay: 0.5 m per scan along x"""
    n, step = 8, 0.5
    mp = synthetic.sequence_map(n, step, **KW)
    truth, scans = [], []
    for i in range(n):
        world = synthetic.lidar_scan(100 + i, x_offset=step * i, **KW)
        T = LR.perturbation(step * i, 0.0, 0.0, 0.0)
        scans.append(np.c_[world[:, :3].astype(np.float64) - T[:3, 3], world[:, 3]].astype(np.float32))
        truth.append(T)
    return mp, truth, scans


def test_the_loop_with_the_cvm_filter_on_the_device_and_the_host_path(sequence):
    """with the true initial velocity every frame's guess is within half a step of the true pose (the loop without an
    estimator starts every one of its first frames a whole step behind), and the two paths hand on the same bits"""
    from sps_amd.localiser import LocalisationLoop, NDTLocaliser
    from sps_amd.sps_filters import SPSCVMFilter
    mp, truth, scans = sequence
    net = net_from_params(O.random_params(seed=0)).cuda().eval().freeze()
    mpt = torch.from_numpy(np.ascontiguousarray(mp[:, :3], dtype=np.float32))
    ndt = NDTLocaliser(mp[:, :3].astype(np.float64), resolution=RES, leaf=LEAF)
    imu = synthetic.sequence_imu(len(scans), step=0.5, scan_period=0.1, rate=100.0)

    def run(device_guess, estimator_on=True):
        est = estimator(truth[0], (5.0, 0.0, 0.0)) if estimator_on else None
        loop = LocalisationLoop(SPSCVMFilter(net, mpt, voxel_size=CFG["MODEL"]["VOXEL_SIZE"], epsilon=2.0), ndt, truth[0],
                                estimator=est, device_guess=device_guess)
        assert loop.device_guess is bool(device_guess)
        return [loop.step(s, imu=imu[k]) if estimator_on else loop.step(s) for k, s in enumerate(scans)]

    on_dev, on_host = run(True), run(False)
    for k, (a, b) in enumerate(zip(on_dev, on_host)):
        gt = float(np.linalg.norm(a.guess[:3, 3] - truth[k][:3, 3]))
        print(f"frame {k}: guess error {gt:.4f} m  status {a.pose_result.status}/{b.pose_result.status}  pose error "
              f"{np.linalg.norm(a.pose[:3, 3] - truth[k][:3, 3]):.4f} m  estimate error "
              f"{np.linalg.norm(a.estimate[:3, 3] - truth[k][:3, 3]):.4f} m")
        assert gt < 0.25, k
        assert a.guess.tobytes() == b.guess.tobytes(), k
        if not a.flagged and not b.flagged:
            assert a.pose.tobytes() == b.pose.tobytes() and a.estimate.tobytes() == b.estimate.tobytes(), k
            assert a.pose_result.trace.tobytes() == b.pose_result.trace.tobytes(), k
        assert a.batch is not None and b.batch is None
    assert any(not a.flagged and not b.flagged for a, b in zip(on_dev, on_host))
    plain = run(None, estimator_on=False)
    lag = [float(np.linalg.norm(s.guess[:3, 3] - truth[k][:3, 3])) for k, s in enumerate(plain)]
    print("guess error without an estimator:", " ".join(f"{v:.3f}" for v in lag))
    assert lag[1] > 0.25 and all(s.estimate is None for s in plain)
