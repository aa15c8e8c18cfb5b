"""The pose estimator's specification (tests/ukf_reference.py) checked on the CPU: against an independently written
vectorised UKF, against the linear Kalman prediction, and on the properties DESIGN.md 8j states.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import ukf_reference as UR


def rot(yaw=0.0, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


# ---- an independent vectorised UKF: np.linalg.cholesky, matrix products, the full 23 x 23 factor -----------------------
def _qmul(a, b):
    w1, x1, y1, z1 = a.T
    w2, x2, y2, z2 = b.T
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=1)


def vec_predict(x, P, dt, gyro, Q):
    n = 16
    L = np.linalg.cholesky((n + 1.0) * P)
    S = np.vstack([x[None], x[None] + L.T, x[None] - L.T])
    Y = S.copy()
    Y[:, 0:3] = S[:, 0:3] + S[:, 3:6] * dt
    q = S[:, 6:10]
    if gyro is not None:
        h = 0.5 * dt * (np.asarray(gyro)[None] - S[:, 13:16])
        dq = np.hstack([np.ones((len(S), 1)), h])
        q = _qmul(q, dq / np.linalg.norm(dq, axis=1, keepdims=True))
    Y[:, 6:10] = q / np.linalg.norm(q, axis=1, keepdims=True)
    w = np.full(2 * n + 1, 1.0 / (2 * (n + 1.0)))
    w[0] = 1.0 / (n + 1.0)
    mean = w @ Y
    D = Y - mean
    Pn = (D.T * w) @ D + np.diag(np.asarray(Q) * dt)
    mean[6:10] /= np.linalg.norm(mean[6:10])
    return mean, Pn


def vec_correct(x, P, z, R):
    n, k = 16, 7
    ne = n + k
    Pe = np.zeros((ne, ne))
    Pe[:n, :n] = P
    Pe[n:, n:] = np.diag(R)
    L = np.linalg.cholesky((ne + 1.0) * Pe)
    xe = np.concatenate([x, np.zeros(k)])
    S = np.vstack([xe[None], xe[None] + L.T, xe[None] - L.T])
    Z = np.hstack([S[:, 0:3], S[:, 6:10]]) + S[:, n:]
    w = np.full(2 * ne + 1, 1.0 / (2 * (ne + 1.0)))
    w[0] = 1.0 / (ne + 1.0)
    zbar = w @ Z
    DZ, DX = Z - zbar, S[:, :n] - x
    Pz = (DZ.T * w) @ DZ
    Pxz = (DX.T * w) @ DZ
    Kg = Pxz @ np.linalg.inv(Pz)
    z = np.array(z, dtype=np.float64)
    if x[6:10] @ z[3:7] < 0:
        z[3:7] = -z[3:7]
    xn = x + Kg @ (z - zbar)
    Pn = P - Kg @ Pz @ Kg.T
    xn[6:10] /= np.linalg.norm(xn[6:10])
    return xn, Pn, z - zbar


def scenario(reverse=False, vec=False, cycles=6):
    """a rotated start, a gyro turning about a tilted axis, a measurement that disagrees a little: [x | P] per step"""
    T0 = rot(0.4, -0.2, 0.1, (1.0, -2.0, 0.5))
    st = UR.init(T0, (2.0, 0.5, -0.1), 0.01)
    x, P = st.x.copy(), st.P.copy()
    out = []
    for c in range(cycles):
        gyro = (0.1, -0.05, 0.5 + 0.1 * c)
        Tm = rot(0.4 + 0.05 * (c + 1), -0.2, 0.1, (1.0 + 0.2 * (c + 1), -2.0 + 0.06 * (c + 1), 0.5))
        if vec:
            for _ in range(2):
                x, P = vec_predict(x, P, 0.05, gyro, UR.PROCESS_DEFAULT)
            x, P = vec_predict(x, P, 0.02, None, UR.PROCESS_DEFAULT)
            out.append(np.concatenate([x, P.ravel()]))
            x, P, _ = vec_correct(x, P, UR.measurement_of(Tm), UR.MEASUREMENT_DEFAULT)
            out.append(np.concatenate([x, P.ravel()]))
        else:
            info = UR.predict(st, [[0.05, 0, 0, 9.8, *gyro]] * 2, reverse=reverse)
            assert list(info) == [0, 2, -1, 0]
            assert list(UR.predict_dt(st, 0.02, reverse=reverse)) == [0, 1, -1, 0]
            out.append(np.concatenate([st.x, st.P.ravel()]))
            status, _ = UR.correct(st, Tm, reverse=reverse)
            assert status == 0
            out.append(np.concatenate([st.x, st.P.ravel()]))
    return np.array(out)


def test_the_restatement_agrees_with_a_vectorised_ukf():
    fwd, rev, vec = scenario(), scenario(reverse=True), scenario(vec=True)
    spread = float(np.abs(fwd - rev).max())
    tol = max(100.0 * spread, 1e-12)
    err = float(np.abs(fwd - vec).max())
    print(f"summation spread {spread:.3e}  tolerance {tol:.3e}  restatement - vectorised {err:.3e}")
    assert err <= tol
    assert np.abs(fwd).max() > 1.0 and not np.array_equal(fwd[0], fwd[-1])


def test_the_pv_block_is_the_linear_kalman_prediction():
    st = UR.init(rot(0.3), (5.0, 0.0, 0.0), 0.01)
    for c in range(4):                                               # a covariance with cross terms
        UR.predict(st, [[0.1, 0, 0, 0, 0, 0, 0.2]])
        UR.correct(st, rot(0.3 + 0.02 * c, t=(0.5 * (c + 1), 0, 0)))
    dt = 0.1
    F = np.eye(6)
    F[0:3, 3:6] = dt * np.eye(3)
    want = F @ st.P[:6, :6] @ F.T + np.diag(UR.PROCESS_DEFAULT[:6] * dt)
    assert UR.predict(st, [[dt, 0, 0, 0, 0.3, -0.1, 0.2]])[0] == 0
    err = np.abs(st.P[:6, :6] - want).max()
    print(f"(p, v) block - F P F^T - Q dt: {err:.3e} absolute, {err / np.abs(want).max():.3e} relative")
    assert err <= 1e-12 * np.abs(want).max()


def test_a_straight_line_with_the_true_velocity_is_predicted_exactly():
    st = UR.init(np.eye(4), (5.0, 0.0, 0.0))
    for k in range(1, 9):
        assert UR.predict_dt(st, 0.1)[0] == 0
        truth = rot(t=(0.5 * k, 0.0, 0.0))
        err = float(np.linalg.norm(st.T[:3, 3] - truth[:3, 3]))
        assert err < 1e-9, (k, err)
        assert UR.correct(st, truth)[0] == 0


def test_a_zero_velocity_start_learns_the_velocity_slowly():
    """the package's default noises: the guess lags a whole step at frame 1 and still most of one at frame 8"""
    st = UR.init(np.eye(4))
    lag = []
    for k in range(1, 33):
        UR.predict_dt(st, 0.1)
        lag.append(0.5 * k - st.T[0, 3])
        UR.correct(st, rot(t=(0.5 * k, 0.0, 0.0)))
    print("lag at frames 1, 8, 16, 24, 32:", [round(float(lag[k - 1]), 3) for k in (1, 8, 16, 24, 32)])
    assert abs(lag[0] - 0.5) < 1e-12
    for k, want in ((8, 0.45), (16, 0.24), (24, 0.11), (32, 0.05)):
        assert abs(lag[k - 1] - want) < 0.01, (k, lag[k - 1])


def test_minus_q_measures_the_same_bits():
    a = UR.init(rot(2.9, 0.1), (1.0, 0, 0))
    UR.predict(a, [[0.1, 0, 0, 0, 0, 0, 0.3]])
    b = a.copy()
    z = UR.measurement_of(rot(2.95, 0.1, t=(0.1, 0, 0)))
    zn = z.copy()
    zn[3:7] = -zn[3:7]
    sa, na = UR.correct_z(a, z)
    sb, nb = UR.correct_z(b, zn)
    assert sa == sb == 0 and na.tobytes() == nb.tobytes()
    assert a.x.tobytes() == b.x.tobytes() and a.P.tobytes() == b.P.tobytes() and a.T.tobytes() == b.T.tobytes()


def test_p_stays_symmetric_and_positive_definite_over_60_cycles():
    st = UR.init(rot(0.2), (5.0, 0.0, 0.0))
    for k in range(1, 61):
        assert UR.predict(st, [[0.05, 0, 2.5, 0, 0, 0, 0.5]] * 2)[0] == 0
        assert st.P.tobytes() == np.ascontiguousarray(st.P.T).tobytes()
        th = 0.2 + 0.05 * k
        assert UR.correct(st, rot(th, t=(10 * math.sin(th), 10 * (1 - math.cos(th)), 0)))[0] == 0
        assert st.P.tobytes() == np.ascontiguousarray(st.P.T).tobytes()
        assert np.linalg.eigvalsh(st.P).min() > 0
    assert st.predicts == 120 and st.corrects == 60


R90X = np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])                # trace == R00: the tie goes to the trace
R180XY = np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, -1]])             # R00 == R11 > trace: the tie goes to R00
R180YZ = np.array([[-1.0, 0, 0], [0, 0, 1], [0, 1, 0]])             # R11 == R22 > R00 == trace: the tie goes to R11


@pytest.mark.parametrize("R, branch", [(np.eye(3), 0), (rot(0.3, 0.2, 0.1)[:3, :3], 0), (np.diag([1.0, -1, -1]), 1),
                                       (np.diag([-1.0, 1, -1]), 2), (np.diag([-1.0, -1, 1]), 3), (rot(3.0)[:3, :3], 3),
                                       (rot(0, 3.0)[:3, :3], 2), (rot(0, 0, 3.0)[:3, :3], 1), (R90X, 0), (R180XY, 1),
                                       (R180YZ, 2)])
def test_every_shepperd_branch_and_tie(R, branch):
    q, got = UR.quat_from_rotation(R)
    assert got == branch
    assert abs(sum(v * v for v in q) - 1.0) < 4e-16
    x = np.zeros(16)
    x[6:10] = q
    assert np.abs(UR.pose_of(x)[:3, :3] - R).max() < 1e-15


def test_a_negative_variance_is_singular_and_leaves_the_state_alone():
    st = UR.init(rot(0.2), (1.0, 0, 0))
    st.P[4, 4] = -1.0
    before = (st.x.tobytes(), st.P.tobytes(), st.T.tobytes())
    assert list(UR.predict_dt(st, 0.1)) == [3, 0, 0, 0]
    assert list(UR.predict(st, [[0.1] + [0.0] * 6] * 3)) == [3, 0, 0, 0]
    status, nu = UR.correct(st, rot(0.2))
    assert status == 3 and not nu.any()
    assert (st.x.tobytes(), st.P.tobytes(), st.T.tobytes()) == before
    # a sample that fails in the middle: the state of the sample before it, and its index
    good = UR.init(rot(0.2), (1.0, 0, 0))
    want = good.copy()
    UR.predict(want, [[0.1] + [0.0] * 6] * 2)
    info = UR.predict(good, [[0.1] + [0.0] * 6] * 2 + [[0.1, 0, 0, 0, float("nan"), 0, 0]] + [[0.1] + [0.0] * 6])
    assert list(info) == [3, 2, 2, 0] and good.x.tobytes() == want.x.tobytes() and good.P.tobytes() == want.P.tobytes()
    # a closed gate is status 2 and changes nothing; a failed registration's pose is never read
    st = UR.init(rot(0.2))
    before = (st.x.tobytes(), st.P.tobytes())
    assert UR.correct(st, np.full((4, 4), np.nan), gate=2)[0] == 2 and UR.correct(st, rot(0.5), gate=3)[0] == 2
    assert (st.x.tobytes(), st.P.tobytes()) == before
    assert UR.correct(st, rot(0.25), gate=1)[0] == 0 and st.x.tobytes() != before[0]


def test_the_circle_drifts_as_the_model_says():
    """velocity is constant in the world frame: on a 0.5 rad/s, 5 m/s circle with an exact gyro the guess drifts"""
    from sps_amd import synthetic
    poses = synthetic.circle_poses(9, yaw_rate=0.5)
    imu = synthetic.sequence_imu(9, rate=100.0, yaw_rate=0.5)
    st = UR.init(poses[0], (5.0, 0.0, 0.0))
    worst_t = worst_r = 0.0
    for k in range(1, 9):
        assert len(imu[k]) == 10 and UR.predict(st, imu[k])[0] == 0
        worst_t = max(worst_t, float(np.linalg.norm(st.T[:3, 3] - poses[k][:3, 3])))
        c = (np.trace(st.T[:3, :3].T @ poses[k][:3, :3]) - 1.0) / 2.0
        worst_r = max(worst_r, math.degrees(math.acos(min(1.0, c))))
        UR.correct(st, poses[k])
    print(f"circle: worst guess error {worst_t:.3f} m, {worst_r:.3f} deg over 8 frames")
    assert 0.02 < worst_t < 0.3 and worst_r < 1.0


# ---- the binding and the argument checks (no device work is reached) ---------------------------------------------------------
def test_the_binding_and_the_argument_checks():
    from sps_amd import _native
    lib = _native.lib
    for name in ("sps_ukf_state_bytes", "sps_ukf_init", "sps_ukf_predict", "sps_ukf_predict_dt", "sps_ukf_correct"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    assert lib.sps_version() == _native.ABI_VERSION == 202                      # additive: the ABI version does not change
    assert lib.sps_ukf_state_bytes() == (16 + 256 + 16) * 8 + 16 and _native.UKF_MAX_IMU == UR.MAX_IMU == 256
    ok16, ok7 = (C.c_double * 16)(*[1.0] * 16), (C.c_double * 7)(*[0.01] * 7)
    bad16, neg7 = (C.c_double * 16)(*([1.0] * 15 + [float("nan")])), (C.c_double * 7)(*([0.01] * 6 + [-1.0]))
    eye = (C.c_double * 16)(*np.eye(4).ravel())
    nan_pose = (C.c_double * 16)(*([float("inf")] + [0.0] * 15))
    fake = 4096                                                                # never dereferenced: every call is refused first
    INVALID = _native.ERR_INVALID
    assert lib.sps_ukf_init(None, eye, None, ok16, None) == INVALID
    assert lib.sps_ukf_init(fake, nan_pose, None, ok16, None) == INVALID
    assert lib.sps_ukf_init(fake, eye, None, bad16, None) == INVALID
    assert lib.sps_ukf_predict(fake, fake, 257, ok16, None, None, None) == INVALID
    assert lib.sps_ukf_predict(fake, fake, -1, ok16, None, None, None) == INVALID
    assert lib.sps_ukf_predict(fake, None, 1, ok16, None, None, None) == INVALID
    assert lib.sps_ukf_predict(fake, fake, 1, bad16, None, None, None) == INVALID
    for dt in (0.0, -0.1, float("nan"), float("inf")):
        assert lib.sps_ukf_predict_dt(fake, dt, ok16, None, None, None) == INVALID
    assert lib.sps_ukf_predict_dt(None, 0.1, ok16, None, None, None) == INVALID
    assert lib.sps_ukf_correct(fake, None, None, ok7, None, None) == INVALID
    assert lib.sps_ukf_correct(fake, fake, None, neg7, None, None) == INVALID
    assert b"meas_diag" in lib.sps_last_error()


def test_python_errors_come_before_any_device_work():
    """device="nowhere:0" is never looked at: every one of these is refused first"""
    from sps_amd.pose_estimator import PoseEstimator, checked_imu
    with pytest.raises(ValueError):
        PoseEstimator(np.eye(3), "nowhere:0")
    with pytest.raises(ValueError):
        PoseEstimator(np.full((4, 4), np.nan), "nowhere:0")
    with pytest.raises(ValueError):
        PoseEstimator(np.eye(4), "nowhere:0", initial_velocity=(1.0, 2.0))
    with pytest.raises(ValueError):
        PoseEstimator(np.eye(4), "nowhere:0", initial_cov=-1.0)
    with pytest.raises(ValueError):
        PoseEstimator(np.eye(4), "nowhere:0", process_noise=[1.0] * 15)
    with pytest.raises(ValueError):
        PoseEstimator(np.eye(4), "nowhere:0", measurement_noise=[float("nan")] * 7)
    for bad in ([[0.1] * 6], [[0.0] + [0.0] * 6], [[0.1, 0, 0, 0, float("nan"), 0, 0]], [[-0.1] + [0.0] * 6]):
        with pytest.raises(ValueError):
            checked_imu(bad)
    assert checked_imu([]).shape == (0, 7) and checked_imu([[0.1] + [0.0] * 6]).shape == (1, 7)


def test_the_loop_refuses_what_it_cannot_do_with_an_estimator():
    from sps_amd.localiser import LocalisationLoop, LoopStep

    class TakesPose:
        pass

    class TakesNone:
        takes_pose = False

    class Est:
        pose_dev = None

        def predict(self, dt): ...
        def predict_imu(self, s): ...
        def correct_from(self, p): ...
        def snapshot(self): ...

    class Ndt:
        resolutions = None

        def submit_from_device(self, *a, **k): ...
        def submit_batch(self, *a, **k): ...

    class Pyr(Ndt):
        resolutions = (2.0, 1.0)

    with pytest.raises(ValueError):
        LocalisationLoop(TakesNone(), Ndt(), np.eye(4), device_guess=True)                      # no estimator
    with pytest.raises(TypeError):
        LocalisationLoop(TakesNone(), Ndt(), np.eye(4), estimator=object())
    for f, l, kw in ((TakesPose(), Ndt(), {}), (TakesNone(), Pyr(), {}), (TakesNone(), object(), {}),
                     (TakesNone(), Ndt(), dict(hypotheses=np.eye(4)[None]))):
        with pytest.raises(ValueError):
            LocalisationLoop(f, l, np.eye(4), estimator=Est(), device_guess=True, **kw)
        assert LocalisationLoop(f, l, np.eye(4), estimator=Est(), **kw).device_guess is False
    assert LocalisationLoop(TakesNone(), Ndt(), np.eye(4), estimator=Est()).device_guess is True
    assert LocalisationLoop(TakesNone(), Ndt(), np.eye(4), estimator=Est(), device_guess=False).device_guess is False
    loop = LocalisationLoop(TakesNone(), Ndt(), np.eye(4))
    with pytest.raises(ValueError):
        loop.step(None, dt=0.1)
    assert LoopStep(None, None, None, None, False).estimate is None


def test_the_synthetic_imu_rows():
    from sps_amd import synthetic
    imu = synthetic.sequence_imu(4, step=0.5, scan_period=0.1, rate=100.0)
    assert [len(r) for r in imu] == [0, 10, 10, 10] and not imu[1][:, 1:].any() and np.all(imu[1][:, 0] == 0.01)
    turn = synthetic.sequence_imu(3, rate=25.0, yaw_rate=0.5)
    assert turn[1].shape == (2, 7) and np.all(turn[1][:, 6] == 0.5) and np.all(turn[1][:, 2] == 2.5) and np.all(turn[1][:, 0] == 0.05)
    p = synthetic.circle_poses(3, yaw_rate=0.5)
    assert np.allclose(p[0], np.eye(4)) and abs(np.linalg.norm(p[1][:3, 3]) - 2 * 10 * math.sin(0.025)) < 1e-12
