// loc_match_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block): the entry points of the scan-matching
// status (ABI: the "localiser, scan-matching status" section of include/sps_hip.h; kernels: loc_match_kernels.inc.h).  The
// call neither allocates nor synchronises; its scratch is the caller's.

int64_t sps_loc_match_status_scratch(int64_t cap) {
  if (cap < 0 || cap > SPS_MAX_POINTS) return -1;
  return loc_align_blocks(cap) * 16 + 16;      // a double and two int32 per workgroup
}

int sps_loc_match_status(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_dev,
                         const int32_t *gate_in_dev, double max_distance, double max_range, double min_inlier_fraction,
                         double max_error, int min_valid, double *out_dev, double *d2_dev, void *scratch_dev, void *stream) {
  if (!c || !n_dev || !T_dev || !out_dev || !scratch_dev || cap < 0 || (cap > 0 && !pts_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (cap > SPS_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_MAX_POINTS);
  if (!c->rg.h.keys) return fail(SPS_ERR_INVALID, "sps_radius_grid_upload has not been called");
  if (!std::isfinite(max_distance) || !(max_distance > 0.0) || max_distance > c->rg.cell_size)
    return fail(SPS_ERR_INVALID, "max_distance must be finite, > 0 and at most the grid's cell size");
  if (std::isnan(max_range) || std::isnan(min_inlier_fraction) || std::isnan(max_error) || min_valid < 0)
    return fail(SPS_ERR_INVALID, "thresholds must not be NaN and min_valid must be >= 0");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)loc_align_blocks(cap);
  double *row_sum = (double *)scratch_dev;
  int *row_cnt = (int *)(row_sum + nb);
  LocMatchArgs a;
  a.md2 = max_distance * max_distance;
  a.mr2 = max_range < 0.0 ? -1.0 : max_range * max_range;
  a.min_fraction = min_inlier_fraction, a.max_error = max_error, a.min_valid = min_valid;
  hipLaunchKernelGGL(k_loc_match<SPS_LOC_MATCH_LANES>, dim3(nb), dim3(256), 0, st, pts_dev, n_dev, (int)cap, c->rg, T_dev, a, d2_dev,
                     row_sum, row_cnt);
  hipLaunchKernelGGL(k_loc_match_final, dim3(1), dim3(64), 0, st, (const double *)row_sum, (const int *)row_cnt, n_dev, (int)cap,
                     gate_in_dev, a, out_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
