// ukf_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block): the C ABI of the pose estimator
// (kernels: ukf_kernels.inc.h; ABI: the "pose estimator" section of include/sps_hip.h).  The state block is the
// caller's; no entry needs a context, allocates, or synchronises.

static_assert(UKF_STATE_DOUBLES * sizeof(double) == SPS_UKF_STATE_BYTES, "the header's state block is the kernels'");

static bool ukf_diag_ok(const double *d, int n) {
  for (int i = 0; i < n; ++i)
    if (!(std::isfinite(d[i]) && d[i] >= 0.0)) return false;
  return true;
}

int64_t sps_ukf_state_bytes(void) { return (int64_t)SPS_UKF_STATE_BYTES; }

int sps_ukf_init(double *state_dev, const double *T_host, const double *v_host, const double *p0_diag, void *stream) {
  if (!state_dev || !T_host || !p0_diag) return fail(SPS_ERR_INVALID, "sps_ukf_init: null argument");
  UkfInit in{};
  for (int i = 0; i < 16; ++i) {
    if (!std::isfinite(T_host[i])) return fail(SPS_ERR_INVALID, "sps_ukf_init: the pose is not finite");
    in.T[i] = T_host[i];
  }
  for (int i = 0; i < 3; ++i) {
    in.vel[i] = v_host ? v_host[i] : 0.0;
    if (!std::isfinite(in.vel[i])) return fail(SPS_ERR_INVALID, "sps_ukf_init: the velocity is not finite");
  }
  if (!ukf_diag_ok(p0_diag, UKF_N)) return fail(SPS_ERR_INVALID, "sps_ukf_init: p0_diag must be finite and >= 0");
  for (int i = 0; i < UKF_N; ++i) in.p0[i] = p0_diag[i];
  hipLaunchKernelGGL(k_ukf_init, dim3(1), dim3(UKF_WG), 0, (hipStream_t)stream, state_dev, in);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

static int ukf_predict_launch(const char *who, double *state_dev, const double *imu_dev, int n, double dt, const double *process_diag_host,
                              double *T_pred_dev, int32_t *info_dev, void *stream) {
  if (!state_dev || !process_diag_host) return fail(SPS_ERR_INVALID, "%s: null argument", who);
  if (!ukf_diag_ok(process_diag_host, UKF_N)) return fail(SPS_ERR_INVALID, "%s: process_diag must be finite and >= 0", who);
  UkfVec Q{};
  for (int i = 0; i < UKF_N; ++i) Q.v[i] = process_diag_host[i];
  hipLaunchKernelGGL(k_ukf_predict, dim3(1), dim3(UKF_WG), 0, (hipStream_t)stream, state_dev, imu_dev, n, dt, Q, T_pred_dev, info_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int sps_ukf_predict(double *state_dev, const double *imu_dev, int32_t n_imu, const double *process_diag_host, double *T_pred_dev,
                    int32_t *info_dev, void *stream) {
  if (n_imu < 0 || n_imu > SPS_UKF_MAX_IMU) return fail(SPS_ERR_INVALID, "sps_ukf_predict: n_imu must be in [0, %d]", SPS_UKF_MAX_IMU);
  if (n_imu > 0 && !imu_dev) return fail(SPS_ERR_INVALID, "sps_ukf_predict: imu_dev is null");
  return ukf_predict_launch("sps_ukf_predict", state_dev, n_imu ? imu_dev : nullptr, n_imu, 0.0, process_diag_host, T_pred_dev, info_dev,
                            stream);
}

int sps_ukf_predict_dt(double *state_dev, double dt, const double *process_diag_host, double *T_pred_dev, int32_t *info_dev,
                       void *stream) {
  if (!(std::isfinite(dt) && dt > 0.0)) return fail(SPS_ERR_INVALID, "sps_ukf_predict_dt: dt must be finite and > 0");
  return ukf_predict_launch("sps_ukf_predict_dt", state_dev, nullptr, 1, dt, process_diag_host, T_pred_dev, info_dev, stream);
}

int sps_ukf_correct(double *state_dev, const double *T_meas_dev, const int32_t *gate_dev, const double *meas_diag_host,
                    double *info_dev, void *stream) {
  if (!state_dev || !T_meas_dev || !meas_diag_host) return fail(SPS_ERR_INVALID, "sps_ukf_correct: null argument");
  if (!ukf_diag_ok(meas_diag_host, UKF_K)) return fail(SPS_ERR_INVALID, "sps_ukf_correct: meas_diag must be finite and >= 0");
  UkfVec R{};
  for (int i = 0; i < UKF_K; ++i) R.v[i] = meas_diag_host[i];
  hipLaunchKernelGGL(k_ukf_correct, dim3(1), dim3(UKF_WG), 0, (hipStream_t)stream, state_dev, T_meas_dev, gate_dev, R, info_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
