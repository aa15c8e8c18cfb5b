// ukf_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace): the pose estimator, an unscented
// Kalman filter over (p, v, q, ba, bg) predicted by the gyroscope and corrected by a registered pose
// (host side: ukf_host.inc.h; ABI: the "pose estimator" section of include/sps_hip.h).
//
//   k_ukf_init      the state block from a pose, a velocity and the diagonal of P
//   k_ukf_predict   every IMU sample of a call in turn (or the one IMU-less step), one launch
//   k_ukf_correct   the correction with a pose on the device, gated by a status on the device
//
// One workgroup of one wave per call; the state is staged in LDS.  The dependent f64 chains are spread over the lanes:
// the Cholesky factor column by column with the rows of a column on different lanes, one sigma point per lane through
// the process model, and a fixed set of entries of every moment per lane.  The arithmetic is loc_kernels.inc.h's: every
// operation rounded on its own (loc_add, loc_mul, __ddiv_rn, __dsqrt_rn), no transcendental function, no float atomic;
// every entry of every sum is summed by one lane in a written order, so the launch geometry cannot change a bit and
// tests/ukf_reference.py agrees bit for bit.

#pragma clang fp contract(off)

constexpr int UKF_N = 16;                  // p 0:3, v 3:6, q 6:10 (w, x, y, z), ba 10:13, bg 13:16
constexpr int UKF_K = 7;                   // measurement: p, q
constexpr int UKF_NSP = 2 * UKF_N + 1;     // sigma points of the prediction
constexpr int UKF_NSC = 2 * (UKF_N + UKF_K) + 1;   // ... of the correction (state extended by the measurement noise)
constexpr int UKF_WG = 64;
constexpr int UKF_TRI = UKF_N * (UKF_N + 1) / 2;
// the state block (doubles): x[16] | P[16][16] | T[16] | int32 (predictions, corrections, 0, 0)
constexpr int UKF_OFF_P = 16, UKF_OFF_T = 272, UKF_OFF_CNT = 288, UKF_STATE_DOUBLES = 290;

struct UkfVec {
  double v[UKF_N];
};
struct UkfInit {
  double T[16], vel[3], p0[UKF_N];
};

struct UkfShared {
  double x[UKF_N], P[UKF_N][UKF_N], A[UKF_N][UKF_N], L[UKF_N][UKF_N], T[16], Q[UKF_N], mean[UKF_N];
  double S[UKF_NSC][UKF_N], D[UKF_NSC][UKF_N], Z[UKF_NSC][UKF_K], DZ[UKF_NSC][UKF_K];
  double z[UKF_K], zbar[UKF_K], nu[UKF_K], sr[UKF_K], Pz[UKF_K][UKF_K], Lz[UKF_K][UKF_K];
  double Pxz[UKF_N][UKF_K], G[UKF_N][UKF_K], M[UKF_N][UKF_K];
  int bad;
};

__device__ inline void ukf_quat_normalise(double q[4]) {
  const double m = __dsqrt_rn(loc_add(loc_add(loc_add(loc_mul(q[0], q[0]), loc_mul(q[1], q[1])), loc_mul(q[2], q[2])), loc_mul(q[3], q[3])));
  for (int a = 0; a < 4; ++a) q[a] = __ddiv_rn(q[a], m);
}

// Shepperd's method on the rotation block of a row-major 4 x 4: the largest of (trace, R00, R11, R22) decides, ties go to
// the first in that order; the result is normalised
__device__ inline void ukf_quat_from_rotation(const double *T, double q[4]) {
  const double r00 = T[0], r01 = T[1], r02 = T[2], r10 = T[4], r11 = T[5], r12 = T[6], r20 = T[8], r21 = T[9], r22 = T[10];
  const double tr = loc_add(loc_add(r00, r11), r22);
  const double cand[4] = {tr, r00, r11, r22};
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (cand[k] > cand[best]) best = k;
  if (best == 0) {
    const double r = __dsqrt_rn(loc_add(1.0, tr));
    const double f = __ddiv_rn(0.5, r);
    q[0] = loc_mul(0.5, r), q[1] = loc_mul(loc_add(r21, -r12), f), q[2] = loc_mul(loc_add(r02, -r20), f), q[3] = loc_mul(loc_add(r10, -r01), f);
  } else if (best == 1) {
    const double r = __dsqrt_rn(loc_add(loc_add(loc_add(1.0, r00), -r11), -r22));
    const double f = __ddiv_rn(0.5, r);
    q[0] = loc_mul(loc_add(r21, -r12), f), q[1] = loc_mul(0.5, r), q[2] = loc_mul(loc_add(r01, r10), f), q[3] = loc_mul(loc_add(r02, r20), f);
  } else if (best == 2) {
    const double r = __dsqrt_rn(loc_add(loc_add(loc_add(1.0, -r00), r11), -r22));
    const double f = __ddiv_rn(0.5, r);
    q[0] = loc_mul(loc_add(r02, -r20), f), q[1] = loc_mul(loc_add(r01, r10), f), q[2] = loc_mul(0.5, r), q[3] = loc_mul(loc_add(r12, r21), f);
  } else {
    const double r = __dsqrt_rn(loc_add(loc_add(loc_add(1.0, -r00), -r11), r22));
    const double f = __ddiv_rn(0.5, r);
    q[0] = loc_mul(loc_add(r10, -r01), f), q[1] = loc_mul(loc_add(r02, r20), f), q[2] = loc_mul(loc_add(r12, r21), f), q[3] = loc_mul(0.5, r);
  }
  ukf_quat_normalise(q);
}

// the 4 x 4 pose of a mean: the rotation of its (unit) quaternion and its position
__device__ inline void ukf_pose_of(const double *x, double *T) {
  const double w = x[6], qx = x[7], qy = x[8], qz = x[9];
  const double xx = loc_mul(qx, qx), yy = loc_mul(qy, qy), zz = loc_mul(qz, qz);
  const double xy = loc_mul(qx, qy), xz = loc_mul(qx, qz), yz = loc_mul(qy, qz);
  const double wx = loc_mul(w, qx), wy = loc_mul(w, qy), wz = loc_mul(w, qz);
  T[0] = loc_add(1.0, -loc_mul(2.0, loc_add(yy, zz))), T[1] = loc_mul(2.0, loc_add(xy, -wz)), T[2] = loc_mul(2.0, loc_add(xz, wy));
  T[4] = loc_mul(2.0, loc_add(xy, wz)), T[5] = loc_add(1.0, -loc_mul(2.0, loc_add(xx, zz))), T[6] = loc_mul(2.0, loc_add(yz, -wx));
  T[8] = loc_mul(2.0, loc_add(xz, -wy)), T[9] = loc_mul(2.0, loc_add(yz, wx)), T[10] = loc_add(1.0, -loc_mul(2.0, loc_add(xx, yy)));
  T[3] = x[0], T[7] = x[1], T[11] = x[2];
  T[12] = 0.0, T[13] = 0.0, T[14] = 0.0, T[15] = 1.0;
}

// Lower Cholesky factor of the lower triangle of A (LDS, n x n), column by column: every lane forms the pivot of the
// column (the same bits on all of them, so the verdict is uniform), lane i > j the entry of row i; inner sums in ascending
// index.  L's upper triangle is left alone.  False where a pivot is not > 0.  Ends behind a barrier.
template <int n>
__device__ inline bool ukf_cholesky(const double (*A)[n], double (*L)[n], int t) {
  for (int j = 0; j < n; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d = loc_add(d, -loc_mul(L[j][k], L[j][k]));
    if (!(d > 0.0)) return false;
    const double ljj = __dsqrt_rn(d);
    if (t == j) {
      L[j][j] = ljj;
    } else if (t > j && t < n) {
      double s = A[t][j];
      for (int k = 0; k < j; ++k) s = loc_add(s, -loc_mul(L[t][k], L[j][k]));
      L[t][j] = __ddiv_rn(s, ljj);
    }
    __syncthreads();
  }
  return true;
}

// entry e of a lower triangle in row order -> (i, j), i >= j
__device__ inline void ukf_tri(int e, int &i, int &j) {
  i = 0;
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  j = e - i * (i + 1) / 2;
}

__device__ inline void ukf_load(UkfShared &sh, const double *state, int t) {
  if (t < UKF_N) sh.x[t] = state[t], sh.T[t] = state[UKF_OFF_T + t];
  for (int e = t; e < UKF_N * UKF_N; e += UKF_WG) (&sh.P[0][0])[e] = state[UKF_OFF_P + e];
}

// sh.x, sh.P and sh.T into the state block
__device__ inline void ukf_store(const UkfShared &sh, double *state, int t) {
  if (t < UKF_N) state[t] = sh.x[t], state[UKF_OFF_T + t] = sh.T[t];
  for (int e = t; e < UKF_N * UKF_N; e += UKF_WG) state[UKF_OFF_P + e] = (&sh.P[0][0])[e];
}

// sh.x / sh.P / sh.T = sh.mean / the lower triangle of sh.A mirrored / the mean's pose.  Ends behind a barrier.
__device__ inline void ukf_commit(UkfShared &sh, int t) {
  if (t < UKF_N) sh.x[t] = sh.mean[t];
  for (int e = t; e < UKF_N * UKF_N; e += UKF_WG) {
    const int i = e >> 4, j = e & 15;
    sh.P[i][j] = i >= j ? sh.A[i][j] : sh.A[j][i];
  }
  if (t == 0) ukf_pose_of(sh.mean, sh.T);
  __syncthreads();
}

// One prediction of the state in LDS (has_imu false: g is ignored and q' = q / |q|).  Uniform result; false leaves
// sh.x, sh.P and sh.T as they were.  Enters and leaves behind a barrier.
__device__ inline bool ukf_predict_step(UkfShared &sh, int t, double dt, const double g[3], bool has_imu) {
  constexpr double N1 = 17.0, W0 = 1.0 / 17.0, W1 = 1.0 / 34.0;
  for (int e = t; e < UKF_N * UKF_N; e += UKF_WG) {
    (&sh.A[0][0])[e] = loc_mul(N1, (&sh.P[0][0])[e]);
    (&sh.L[0][0])[e] = 0.0;
  }
  if (t == 0) sh.bad = 0;
  __syncthreads();
  if (!ukf_cholesky<UKF_N>(sh.A, sh.L, t)) return false;
  if (t < UKF_NSP) {  // sigma point t: x, x + L[:, t - 1], x - L[:, t - 17], then through f
    double s[UKF_N];
    for (int r = 0; r < UKF_N; ++r) {
      double v = sh.x[r];
      if (t >= 1 && t <= UKF_N) v = loc_add(v, sh.L[r][t - 1]);
      if (t > UKF_N) v = loc_add(v, -sh.L[r][t - 1 - UKF_N]);
      s[r] = v;
    }
    for (int a = 0; a < 3; ++a) s[a] = loc_add(s[a], loc_mul(s[3 + a], dt));
    double q[4] = {s[6], s[7], s[8], s[9]};
    if (has_imu) {
      const double hdt = loc_mul(0.5, dt);
      double h[3];
      for (int a = 0; a < 3; ++a) h[a] = loc_mul(hdt, loc_add(g[a], -s[13 + a]));
      const double nrm = __dsqrt_rn(loc_add(loc_add(loc_add(1.0, loc_mul(h[0], h[0])), loc_mul(h[1], h[1])), loc_mul(h[2], h[2])));
      const double dw = __ddiv_rn(1.0, nrm), dx = __ddiv_rn(h[0], nrm), dy = __ddiv_rn(h[1], nrm), dz = __ddiv_rn(h[2], nrm);
      const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
      q[0] = loc_add(loc_add(loc_add(loc_mul(qw, dw), -loc_mul(qx, dx)), -loc_mul(qy, dy)), -loc_mul(qz, dz));
      q[1] = loc_add(loc_add(loc_add(loc_mul(qw, dx), loc_mul(qx, dw)), loc_mul(qy, dz)), -loc_mul(qz, dy));
      q[2] = loc_add(loc_add(loc_add(loc_mul(qw, dy), -loc_mul(qx, dz)), loc_mul(qy, dw)), loc_mul(qz, dx));
      q[3] = loc_add(loc_add(loc_add(loc_mul(qw, dz), loc_mul(qx, dy)), -loc_mul(qy, dx)), loc_mul(qz, dw));
    }
    ukf_quat_normalise(q);
    for (int a = 0; a < 4; ++a) s[6 + a] = q[a];
    for (int r = 0; r < UKF_N; ++r) sh.S[t][r] = s[r];
  }
  __syncthreads();
  if (t < UKF_N) {
    double m = loc_mul(W0, sh.S[0][t]);
    for (int s = 1; s < UKF_NSP; ++s) m = loc_add(m, loc_mul(W1, sh.S[s][t]));
    sh.mean[t] = m;
  }
  __syncthreads();
  if (t < UKF_NSP)
    for (int r = 0; r < UKF_N; ++r) sh.D[t][r] = loc_add(sh.S[t][r], -sh.mean[r]);
  __syncthreads();
  for (int e = t; e < UKF_TRI; e += UKF_WG) {
    int i, j;
    ukf_tri(e, i, j);
    double c = 0.0;
    for (int s = 0; s < UKF_NSP; ++s) c = loc_add(c, loc_mul(s == 0 ? W0 : W1, loc_mul(sh.D[s][i], sh.D[s][j])));
    if (i == j) c = loc_add(c, loc_mul(sh.Q[i], dt));
    sh.A[i][j] = c;
    if (!isfinite(c)) sh.bad = 1;
  }
  if (t == 0) {  // the mean's quaternion, renormalised behind the covariance (which is about the mean as summed)
    double q[4] = {sh.mean[6], sh.mean[7], sh.mean[8], sh.mean[9]};
    ukf_quat_normalise(q);
    for (int a = 0; a < 4; ++a) sh.mean[6 + a] = q[a];
    for (int r = 0; r < UKF_N; ++r)
      if (!isfinite(sh.mean[r])) sh.bad = 1;
  }
  __syncthreads();
  if (sh.bad) return false;
  ukf_commit(sh, t);
  return true;
}

__global__ __launch_bounds__(UKF_WG) void k_ukf_init(double *__restrict__ state, UkfInit in) {
  __shared__ double x[UKF_N], T[16];
  const int t = threadIdx.x;
  if (t == 0) {
    double q[4];
    ukf_quat_from_rotation(in.T, q);
    x[0] = in.T[3], x[1] = in.T[7], x[2] = in.T[11];
    for (int a = 0; a < 3; ++a) x[3 + a] = in.vel[a];
    for (int a = 0; a < 4; ++a) x[6 + a] = q[a];
    for (int a = 10; a < UKF_N; ++a) x[a] = 0.0;
    ukf_pose_of(x, T);
  }
  __syncthreads();
  if (t < UKF_N) state[t] = x[t], state[UKF_OFF_T + t] = T[t];
  for (int e = t; e < UKF_N * UKF_N; e += UKF_WG) state[UKF_OFF_P + e] = (e >> 4) == (e & 15) ? in.p0[e >> 4] : 0.0;
  if (t < 4) reinterpret_cast<int *>(state + UKF_OFF_CNT)[t] = 0;
}

// imu: [n][7] rows (dt, ax, ay, az, gx, gy, gz), or null: n is then 1 and the one step is the IMU-less one over dt_only.
// info: int32 (status, samples done, failing sample or -1, 0).
__global__ __launch_bounds__(UKF_WG) void k_ukf_predict(double *__restrict__ state, const double *__restrict__ imu, int n,
                                                        double dt_only, UkfVec Q, double *__restrict__ T_pred,
                                                        int *__restrict__ info) {
  __shared__ UkfShared sh;
  const int t = threadIdx.x;
  ukf_load(sh, state, t);
  if (t < UKF_N) sh.Q[t] = Q.v[t];
  __syncthreads();
  int done = 0, bad = -1;
  for (int j = 0; j < n; ++j) {  // everything that decides is uniform: all lanes read the same row
    double dt = dt_only, g[3] = {0.0, 0.0, 0.0};
    bool ok = true;
    if (imu) {
      const double *row = imu + (size_t)j * 7;
      dt = row[0];
      for (int a = 1; a < 7; ++a) ok = ok && isfinite(row[a]);
      g[0] = row[4], g[1] = row[5], g[2] = row[6];
    }
    ok = ok && isfinite(dt) && dt > 0.0;
    if (!ok || !ukf_predict_step(sh, t, dt, g, imu != nullptr)) {
      bad = j;
      break;
    }
    ++done;
  }
  if (done > 0) {
    ukf_store(sh, state, t);
    if (t == 0) reinterpret_cast<int *>(state + UKF_OFF_CNT)[0] += done;
  }
  if (T_pred && t < 16) T_pred[t] = sh.T[t];
  if (info && t == 0) info[0] = bad >= 0 ? 3 : 0, info[1] = done, info[2] = bad, info[3] = 0;
}

// info: 8 doubles, the first one's two int32 halves (status, 0), then the innovation z - zbar (zeros unless status 0)
__device__ inline void ukf_correct_info(double *info, int t, int status, const double *nu) {
  if (!info) return;
  if (t == 0) {
    int *w = reinterpret_cast<int *>(info);
    w[0] = status, w[1] = 0;
  }
  if (t < UKF_K) info[1 + t] = nu ? nu[t] : 0.0;
}

__global__ __launch_bounds__(UKF_WG) void k_ukf_correct(double *__restrict__ state, const double *__restrict__ T_meas,
                                                        const int *__restrict__ gate, UkfVec R, double *__restrict__ info) {
  constexpr double N1 = 24.0, W0 = 1.0 / 24.0, W1 = 1.0 / 48.0;
  __shared__ UkfShared sh;
  const int t = threadIdx.x;
  if (gate) {
    const int gv = *gate;
    if (gv != 0 && gv != 1) {  // the registration failed: nothing of the state block is written
      ukf_correct_info(info, t, 2, nullptr);
      return;
    }
  }
  ukf_load(sh, state, t);
  double Tm[12];
  bool ok = true;
  for (int a = 0; a < 12; ++a) Tm[a] = T_meas[a], ok = ok && isfinite(Tm[a]);
  for (int a = 12; a < 16; ++a) ok = ok && isfinite(T_meas[a]);
  for (int e = t; e < UKF_N * UKF_N; e += UKF_WG) (&sh.L[0][0])[e] = 0.0;
  if (t < UKF_K * UKF_K) (&sh.Lz[0][0])[t] = 0.0;
  if (t == 0) sh.bad = 0;
  __syncthreads();
  for (int e = t; e < UKF_N * UKF_N; e += UKF_WG) (&sh.A[0][0])[e] = loc_mul(N1, (&sh.P[0][0])[e]);
  double sr[UKF_K];
  for (int k = 0; k < UKF_K; ++k) {
    const double v = loc_mul(N1, R.v[k]);
    ok = ok && v >= 0.0;
    sr[k] = __dsqrt_rn(v);
  }
  if (!ok) {  // uniform
    ukf_correct_info(info, t, 3, nullptr);
    return;
  }
  if (t == 0) {  // the measurement z = (p, q), q on the mean's side of the sphere
    double q[4];
    ukf_quat_from_rotation(Tm, q);
    const double dot = loc_add(loc_add(loc_add(loc_mul(sh.x[6], q[0]), loc_mul(sh.x[7], q[1])), loc_mul(sh.x[8], q[2])), loc_mul(sh.x[9], q[3]));
    sh.z[0] = Tm[3], sh.z[1] = Tm[7], sh.z[2] = Tm[11];
    for (int a = 0; a < 4; ++a) sh.z[3 + a] = dot < 0.0 ? -q[a] : q[a];
  }
  __syncthreads();
  if (!ukf_cholesky<UKF_N>(sh.A, sh.L, t)) {
    ukf_correct_info(info, t, 3, nullptr);
    return;
  }
  // sigma point t of the extended state (x, 0): 0 | + column t - 1 (16 of L, then 7 of the noise) | - column t - 24
  if (t < UKF_NSC) {
    const int c = t == 0 ? -1 : (t - 1) % (UKF_N + UKF_K);
    const bool minus = t > UKF_N + UKF_K;
    for (int r = 0; r < UKF_N; ++r) {
      double v = sh.x[r];
      if (c >= 0 && c < UKF_N) v = loc_add(v, minus ? -sh.L[r][c] : sh.L[r][c]);
      sh.S[t][r] = v;
    }
    for (int k = 0; k < UKF_K; ++k) {
      const double e = c == UKF_N + k ? (minus ? -sr[k] : sr[k]) : 0.0;
      sh.Z[t][k] = loc_add(sh.S[t][k < 3 ? k : 3 + k], e);
    }
  }
  __syncthreads();
  if (t < UKF_K) {
    double m = loc_mul(W0, sh.Z[0][t]);
    for (int s = 1; s < UKF_NSC; ++s) m = loc_add(m, loc_mul(W1, sh.Z[s][t]));
    sh.zbar[t] = m;
  }
  __syncthreads();
  if (t < UKF_NSC) {
    for (int k = 0; k < UKF_K; ++k) sh.DZ[t][k] = loc_add(sh.Z[t][k], -sh.zbar[k]);
    for (int r = 0; r < UKF_N; ++r) sh.D[t][r] = loc_add(sh.S[t][r], -sh.x[r]);
  }
  __syncthreads();
  constexpr int TRI_Z = UKF_K * (UKF_K + 1) / 2;
  for (int e = t; e < TRI_Z + UKF_N * UKF_K; e += UKF_WG) {  // Pz (lower triangle, mirrored) and Pxz, one entry per turn
    double c = 0.0;
    if (e < TRI_Z) {
      int a, b;
      ukf_tri(e, a, b);
      for (int s = 0; s < UKF_NSC; ++s) c = loc_add(c, loc_mul(s == 0 ? W0 : W1, loc_mul(sh.DZ[s][a], sh.DZ[s][b])));
      sh.Pz[a][b] = c, sh.Pz[b][a] = c;
    } else {
      const int i = (e - TRI_Z) / UKF_K, k = (e - TRI_Z) % UKF_K;
      for (int s = 0; s < UKF_NSC; ++s) c = loc_add(c, loc_mul(s == 0 ? W0 : W1, loc_mul(sh.D[s][i], sh.DZ[s][k])));
      sh.Pxz[i][k] = c;
    }
  }
  __syncthreads();
  if (!ukf_cholesky<UKF_K>(sh.Pz, sh.Lz, t)) {
    ukf_correct_info(info, t, 3, nullptr);
    return;
  }
  if (t < UKF_N) {  // row t of the gain K = Pxz Pz^-1: Lz y = Pxz[t], Lz^T g = y
    double y[UKF_K], g[UKF_K];
    for (int a = 0; a < UKF_K; ++a) {
      double s = sh.Pxz[t][a];
      for (int k = 0; k < a; ++k) s = loc_add(s, -loc_mul(sh.Lz[a][k], y[k]));
      y[a] = __ddiv_rn(s, sh.Lz[a][a]);
    }
    for (int a = UKF_K - 1; a >= 0; --a) {
      double s = y[a];
      for (int k = a + 1; k < UKF_K; ++k) s = loc_add(s, -loc_mul(sh.Lz[k][a], g[k]));
      g[a] = __ddiv_rn(s, sh.Lz[a][a]);
    }
    for (int a = 0; a < UKF_K; ++a) sh.G[t][a] = g[a];
  }
  if (t < UKF_K) sh.nu[t] = loc_add(sh.z[t], -sh.zbar[t]);
  __syncthreads();
  if (t < UKF_N) {
    double v = sh.x[t];
    for (int k = 0; k < UKF_K; ++k) v = loc_add(v, loc_mul(sh.G[t][k], sh.nu[k]));
    sh.mean[t] = v;
  }
  for (int e = t; e < UKF_N * UKF_K; e += UKF_WG) {  // M = K Pz
    const int i = e / UKF_K, k = e % UKF_K;
    double m = 0.0;
    for (int b = 0; b < UKF_K; ++b) m = loc_add(m, loc_mul(sh.G[i][b], sh.Pz[b][k]));
    sh.M[i][k] = m;
  }
  __syncthreads();
  for (int e = t; e < UKF_TRI; e += UKF_WG) {  // P - M K^T on the lower triangle
    int i, j;
    ukf_tri(e, i, j);
    double u = 0.0;
    for (int k = 0; k < UKF_K; ++k) u = loc_add(u, loc_mul(sh.M[i][k], sh.G[j][k]));
    const double c = loc_add(sh.P[i][j], -u);
    sh.A[i][j] = c;
    if (!isfinite(c)) sh.bad = 1;
  }
  if (t == 0) {
    double q[4] = {sh.mean[6], sh.mean[7], sh.mean[8], sh.mean[9]};
    ukf_quat_normalise(q);
    for (int a = 0; a < 4; ++a) sh.mean[6 + a] = q[a];
    for (int r = 0; r < UKF_N; ++r)
      if (!isfinite(sh.mean[r])) sh.bad = 1;
  }
  __syncthreads();
  if (sh.bad) {
    ukf_correct_info(info, t, 3, nullptr);
    return;
  }
  ukf_commit(sh, t);
  ukf_store(sh, state, t);
  if (t == 0) reinterpret_cast<int *>(state + UKF_OFF_CNT)[1] += 1;
  ukf_correct_info(info, t, 0, sh.nu);
}
