"""Numpy restatement of the device pose estimator (include/sps_hip.h, "pose estimator"): an unscented
Kalman filter over position, velocity, orientation quaternion (w, x, y, z) and the two IMU biases, predicted by the
gyroscope and corrected by a registered pose.  It is the specification the kernels are tested against and never
touches the native library.

Every floating-point operation is a float64 one rounded on its own, in the order the header states: sigma points in
index order, Cholesky and substitution inner sums in ascending index, every sum started as written below.  Where many
entries are computed at once the numpy operations are element-wise (one rounding each, no product-sum is fused); there
is no np.dot, no matmul and no BLAS call in this file.  There is no transcendental function on this path, so the
kernels and this file agree bit for bit."""
import math

import numpy as np

N = 16                       # state entries: p 0:3, v 3:6, q 6:10 (w, x, y, z), ba 10:13, bg 13:16
K = 7                        # measurement entries: p, q
LAMBDA = 1.0
PROCESS_DEFAULT = np.array([1.0] * 3 + [1.0] * 3 + [0.5] * 4 + [1e-6] * 3 + [1e-6] * 3)
MEASUREMENT_DEFAULT = np.array([0.01] * 3 + [0.001] * 4)
DONE, GATE_CLOSED, SINGULAR = 0, 2, 3
MAX_IMU = 256


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


class State:
    """mean x [16], covariance P [16, 16] (exactly symmetric), pose T [4, 4] of the mean, and the counters"""

    def __init__(self, x, P, T, status=DONE, predicts=0, corrects=0):
        self.x, self.P, self.T = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64), np.array(T, dtype=np.float64)
        self.status, self.predicts, self.corrects = int(status), int(predicts), int(corrects)

    def copy(self):
        return State(self.x, self.P, self.T, self.status, self.predicts, self.corrects)


# ---- quaternions and poses ---------------------------------------------------------------------------------------------
def quat_normalise(q):
    w, x, y, z = (float(v) for v in q)
    m = _sqrt(((w * w + x * x) + y * y) + z * z)
    return [_div(w, m), _div(x, m), _div(y, m), _div(z, m)]


def quat_from_rotation(T):
    """Shepperd's method on the rotation block of a 4 x 4 (or 3 x 3) matrix: the largest of (trace, R00, R11, R22) decides,
    ties go to the first in that order; the result is normalised.  Returns ([w, x, y, z], branch)."""
    R = np.asarray(T, dtype=np.float64)
    r00, r01, r02 = float(R[0, 0]), float(R[0, 1]), float(R[0, 2])
    r10, r11, r12 = float(R[1, 0]), float(R[1, 1]), float(R[1, 2])
    r20, r21, r22 = float(R[2, 0]), float(R[2, 1]), float(R[2, 2])
    tr = (r00 + r11) + r22
    cand = (tr, r00, r11, r22)
    best = 0
    for k in range(1, 4):
        if cand[k] > cand[best]:
            best = k
    if best == 0:
        r = _sqrt(1.0 + tr)
        f = _div(0.5, r)
        q = [0.5 * r, (r21 - r12) * f, (r02 - r20) * f, (r10 - r01) * f]
    elif best == 1:
        r = _sqrt(((1.0 + r00) - r11) - r22)
        f = _div(0.5, r)
        q = [(r21 - r12) * f, 0.5 * r, (r01 + r10) * f, (r02 + r20) * f]
    elif best == 2:
        r = _sqrt(((1.0 - r00) + r11) - r22)
        f = _div(0.5, r)
        q = [(r02 - r20) * f, (r01 + r10) * f, 0.5 * r, (r12 + r21) * f]
    else:
        r = _sqrt(((1.0 - r00) - r11) + r22)
        f = _div(0.5, r)
        q = [(r10 - r01) * f, (r02 + r20) * f, (r12 + r21) * f, 0.5 * r]
    return quat_normalise(q), best


def pose_of(x):
    """4 x 4 pose of a mean: the rotation of its (unit) quaternion and its position"""
    w, qx, qy, qz = (float(v) for v in x[6:10])
    xx, yy, zz = qx * qx, qy * qy, qz * qz
    xy, xz, yz = qx * qy, qx * qz, qy * qz
    wx, wy, wz = w * qx, w * qy, w * qz
    T = np.zeros((4, 4))
    T[0, 0], T[0, 1], T[0, 2] = 1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)
    T[1, 0], T[1, 1], T[1, 2] = 2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)
    T[2, 0], T[2, 1], T[2, 2] = 2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)
    T[0, 3], T[1, 3], T[2, 3], T[3, 3] = x[0], x[1], x[2], 1.0
    return T


def measurement_of(T):
    """z = (p, q) of a 4 x 4 pose"""
    q, _ = quat_from_rotation(T)
    return np.array([T[0][3], T[1][3], T[2][3]] + q, dtype=np.float64)


def init(T, v=(0.0, 0.0, 0.0), p0=0.01):
    x = np.zeros(N)
    x[0:3] = [T[0][3], T[1][3], T[2][3]]
    x[3:6] = v
    x[6:10], _ = quat_from_rotation(T)
    P = np.zeros((N, N))
    P[np.arange(N), np.arange(N)] = np.broadcast_to(np.asarray(p0, dtype=np.float64), (N,))
    return State(x, P, pose_of(x))


# ---- the pieces of the unscented transform -----------------------------------------------------------------------------
def cholesky(A, n, reverse=False):
    """Lower factor of the lower triangle of A [n, n], column by column; inner sums in ascending index (``reverse``:
    descending, for the summation-spread yardstick only).  None where a pivot is not > 0."""
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        ks = range(j - 1, -1, -1) if reverse else range(j)
        d = float(A[j][j])
        for k in ks:
            d = d + -(L[j][k] * L[j][k])
        if not d > 0.0:
            return None
        ljj = _sqrt(d)
        L[j][j] = ljj
        for i in range(j + 1, n):
            s = float(A[i][j])
            for k in ks:
                s = s + -(L[i][k] * L[j][k])
            L[i][j] = _div(s, ljj)
    return np.array(L, dtype=np.float64)


def process(s, gyro, dt):
    """f(x, (a, omega), dt) of one sigma point; gyro None: the IMU-less step"""
    o = np.array(s, dtype=np.float64)
    for a in range(3):
        o[a] = float(s[a]) + float(s[3 + a]) * dt
    if gyro is None:
        o[6:10] = quat_normalise(s[6:10])
        return o
    hdt = 0.5 * dt
    h = [hdt * (float(gyro[a]) - float(s[13 + a])) for a in range(3)]
    nrm = _sqrt(((1.0 + h[0] * h[0]) + h[1] * h[1]) + h[2] * h[2])
    dw, dx, dy, dz = _div(1.0, nrm), _div(h[0], nrm), _div(h[1], nrm), _div(h[2], nrm)
    qw, qx, qy, qz = (float(v) for v in s[6:10])
    o[6:10] = quat_normalise([((qw * dw - qx * dx) - qy * dy) - qz * dz,
                              ((qw * dx + qx * dw) + qy * dz) - qz * dy,
                              ((qw * dy - qx * dz) + qy * dw) + qz * dx,
                              ((qw * dz + qx * dy) - qy * dx) + qz * dw])
    return o


def _sigma_order(S, reverse):
    return range(S - 1, -1, -1) if reverse else range(S)


def weighted_mean(Y, w0, w1, reverse=False):
    """sum_s w_s Y[s] per column, started with the first term, in index order"""
    order = list(_sigma_order(len(Y), reverse))
    m = (w0 if order[0] == 0 else w1) * Y[order[0]]
    for s in order[1:]:
        m = m + (w0 if s == 0 else w1) * Y[s]
    return m


def weighted_outer(A, B, w0, w1, reverse=False):
    """sum_s w_s (A[s] B[s]^T), every entry started at 0.0, in index order: entry (i, j) is 0 + w (a_i b_j) + ..."""
    c = np.zeros((A.shape[1], B.shape[1]))
    for s in _sigma_order(len(A), reverse):
        c = c + (w0 if s == 0 else w1) * (A[s][:, None] * B[s][None, :])
    return c


def _mirror_lower(M):
    return np.tril(M) + np.tril(M, -1).T


def predict_step(st, dt, gyro, Q, reverse=False):
    """One prediction; returns False (and leaves ``st`` untouched) where the step is singular or not finite."""
    dt = float(dt)
    if not (math.isfinite(dt) and dt > 0.0) or (gyro is not None and not np.isfinite(np.asarray(gyro, dtype=np.float64)).all()):
        return False
    with np.errstate(all="ignore"):
        n1 = N + LAMBDA
        L = cholesky(n1 * st.P, N, reverse)
        if L is None:
            return False
        S = np.empty((2 * N + 1, N))
        S[0] = st.x
        for i in range(N):
            S[1 + i] = st.x + L[:, i]
            S[1 + N + i] = st.x + -L[:, i]
        Y = np.stack([process(S[s], gyro, dt) for s in range(2 * N + 1)])
        w0, w1 = LAMBDA / n1, 1.0 / (2.0 * n1)
        mean = weighted_mean(Y, w0, w1, reverse)
        D = Y + -mean[None, :]
        P = weighted_outer(D, D, w0, w1, reverse)
        P[np.arange(N), np.arange(N)] = P[np.arange(N), np.arange(N)] + np.asarray(Q, dtype=np.float64) * dt
        P = _mirror_lower(P)
        mean[6:10] = quat_normalise(mean[6:10])
    if not (np.isfinite(mean).all() and np.isfinite(P).all()):
        return False
    st.x, st.P, st.T = mean, P, pose_of(mean)
    return True


def predict(st, imu, Q=PROCESS_DEFAULT, reverse=False):
    """sps_ukf_predict: every row (dt, ax, ay, az, gx, gy, gz) of ``imu`` [M, 7] in turn -> info (status, samples done,
    index of the failing sample or -1, 0).  M = 0 changes nothing."""
    imu = np.asarray(imu, dtype=np.float64).reshape(-1, 7)
    done, bad = 0, -1
    for j, row in enumerate(imu):
        if not np.isfinite(row).all() or not predict_step(st, row[0], row[4:7], Q, reverse):
            bad = j
            break
        done += 1
    st.status = SINGULAR if bad >= 0 else DONE
    st.predicts += done
    return np.array([st.status, done, bad, 0], dtype=np.int32)


def predict_dt(st, dt, Q=PROCESS_DEFAULT, reverse=False):
    """sps_ukf_predict_dt: the IMU-less step"""
    ok = predict_step(st, dt, None, Q, reverse)
    st.status = DONE if ok else SINGULAR
    st.predicts += 1 if ok else 0
    return np.array([st.status, 1 if ok else 0, -1 if ok else 0, 0], dtype=np.int32)


def correct_z(st, z, R=MEASUREMENT_DEFAULT, gate=None, reverse=False):
    """The correction with z = (p, q) -> (status, innovation [7]); ``gate``: the registration's status, None: always
    correct.  z's quaternion is negated when its dot product with the mean's is negative."""
    nu = np.zeros(K)
    if gate is not None and int(gate) not in (0, 1):
        st.status = GATE_CLOSED
        return GATE_CLOSED, nu
    z = np.array(z, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    ok = bool(np.isfinite(z).all())
    with np.errstate(all="ignore"):
        n1 = N + K + LAMBDA
        L = cholesky(n1 * st.P, N, reverse) if ok else None
        ok = ok and L is not None and bool((n1 * R >= 0.0).all())
        if ok:
            q, zq = st.x[6:10], z[3:7]
            if ((float(q[0]) * float(zq[0]) + float(q[1]) * float(zq[1])) + float(q[2]) * float(zq[2])) + float(q[3]) * float(zq[3]) < 0.0:
                z[3:7] = -zq
            sr = np.array([_sqrt(v) for v in n1 * R])
            ns = 2 * (N + K) + 1
            X = np.tile(st.x, (ns, 1))
            E = np.zeros((ns, K))
            for i in range(N):
                X[1 + i] = st.x + L[:, i]
                X[1 + N + K + i] = st.x + -L[:, i]
            for k in range(K):
                E[1 + N + k, k] = sr[k]
                E[1 + N + K + N + k, k] = -sr[k]
            Z = np.concatenate([X[:, 0:3], X[:, 6:10]], axis=1) + E
            w0, w1 = LAMBDA / n1, 1.0 / (2.0 * n1)
            zbar = weighted_mean(Z, w0, w1, reverse)
            DZ = Z + -zbar[None, :]
            DX = X + -st.x[None, :]
            Pz = _mirror_lower(weighted_outer(DZ, DZ, w0, w1, reverse))
            Pxz = weighted_outer(DX, DZ, w0, w1, reverse)
            Lz = cholesky(Pz, K, reverse)
            ok = Lz is not None
        if ok:
            ks = list(range(K))
            G = np.zeros((N, K))                                     # the gain, row i = Pz^-1 Pxz[i]
            for i in range(N):
                y = [0.0] * K
                for a in range(K):
                    s = float(Pxz[i, a])
                    for k in (reversed(ks[:a]) if reverse else ks[:a]):
                        s = s + -(float(Lz[a, k]) * y[k])
                    y[a] = _div(s, Lz[a, a])
                g = [0.0] * K
                for a in range(K - 1, -1, -1):
                    s = y[a]
                    for k in (reversed(ks[a + 1:]) if reverse else ks[a + 1:]):
                        s = s + -(float(Lz[k, a]) * g[k])
                    g[a] = _div(s, Lz[a, a])
                G[i] = g
            nu = z + -zbar
            kord = ks[::-1] if reverse else ks
            x = st.x.copy()
            for k in kord:
                x = x + G[:, k] * nu[k]
            M = np.zeros((N, K))
            for b in kord:
                M = M + G[:, b][:, None] * Pz[b][None, :]
            U = np.zeros((N, N))
            for k in kord:
                U = U + M[:, k][:, None] * G[:, k][None, :]
            P = _mirror_lower(st.P + -U)
            x[6:10] = quat_normalise(x[6:10])
            ok = bool(np.isfinite(x).all() and np.isfinite(P).all())
    if not ok:
        st.status = SINGULAR
        return SINGULAR, np.zeros(K)
    st.x, st.P, st.T = x, P, pose_of(x)
    st.status = DONE
    st.corrects += 1
    return DONE, nu


def correct(st, T_meas, R=MEASUREMENT_DEFAULT, gate=None, reverse=False):
    """sps_ukf_correct: the correction with the pose T_meas [4, 4]"""
    if gate is not None and int(gate) not in (0, 1):
        return correct_z(st, np.zeros(K), R, gate, reverse)
    T = np.asarray(T_meas, dtype=np.float64)
    if not np.isfinite(T).all():
        st.status = SINGULAR
        return SINGULAR, np.zeros(K)
    return correct_z(st, measurement_of(T), R, gate, reverse)
