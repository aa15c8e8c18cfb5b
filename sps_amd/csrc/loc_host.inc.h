// loc_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block): the entry points of the scan-to-map
// localiser (ABI: the "localiser" section of include/sps_hip.h; kernels: loc_kernels.inc.h).  Neither call synchronises
// with the host; their scratch is the caller's, so they never allocate.

namespace {
inline int64_t loc_ds_hcap(int64_t n_max) { return next_pow2(2 * (n_max < 512 ? 512 : n_max)); }
inline int64_t loc_ds_blocks(int64_t n_max) { return std::max<int64_t>(1, (n_max + SCAN_BLOCK - 1) / SCAN_BLOCK); }
inline int64_t loc_align_blocks(int64_t cap) { return std::max<int64_t>(1, (cap + LOC_PTS - 1) / LOC_PTS); }
}  // namespace

int64_t sps_loc_downsample_scratch(int64_t n_max) {
  if (n_max < 0 || n_max > SPS_MAX_POINTS) return -1;
  return loc_ds_hcap(n_max) * 12 + loc_ds_blocks(n_max) * 4;
}

int64_t sps_loc_align_scratch(int64_t cap) {
  if (cap < 0 || cap > SPS_MAX_POINTS) return -1;
  return loc_align_blocks(cap) * LOC_TERMS * 8 + 16;
}

int sps_loc_downsample(sps_ctx *c, const float *rows_dev, int64_t ld, int64_t n_max, const int32_t *n_dev, double leaf,
                       double *out_xyz_dev, int64_t cap, int32_t *count_dev, void *scratch_dev, void *stream) {
  if (!c || !n_dev || !count_dev || !scratch_dev || n_max < 0 || ld < 3 || cap < 0 || (n_max > 0 && !rows_dev) ||
      (cap > 0 && !out_xyz_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (!(leaf > 0.0) || std::isinf(leaf)) return fail(SPS_ERR_INVALID, "leaf must be finite and > 0");
  if (n_max > SPS_MAX_POINTS || cap > SPS_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_MAX_POINTS);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t hcap = loc_ds_hcap(n_max);
  const int nb = (int)loc_ds_blocks(n_max);
  HashTable h;
  h.keys = (uint64_t *)scratch_dev;
  h.first = (int *)((char *)scratch_dev + hcap * 8);
  h.rank = nullptr;
  h.mask = (uint32_t)(hcap - 1);
  int *block_sums = h.first + hcap;
  HIP_TRY(hipMemsetAsync(h.keys, 0xFF, (size_t)hcap * 8, st));
  HIP_TRY(hipMemsetAsync(h.first, 0x7F, (size_t)hcap * 4, st));   // 0x7F7F7F7F: above every row index
  // an empty input still runs one (empty) workgroup of the two compaction passes: it publishes count = 0
  if (n_max > 0)
    hipLaunchKernelGGL(k_loc_ds_insert, dim3(nb), dim3(SCAN_BLOCK), 0, st, rows_dev, ld, (int)n_max, n_dev, leaf, h);
  hipLaunchKernelGGL(k_loc_ds_count, dim3(nb), dim3(SCAN_BLOCK), 0, st, rows_dev, ld, (int)n_max, n_dev, leaf, h, block_sums);
  hipLaunchKernelGGL(k_loc_ds_write, dim3(nb), dim3(SCAN_BLOCK), 0, st, rows_dev, ld, (int)n_max, n_dev, leaf, h, block_sums,
                     out_xyz_dev, (int)cap, count_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int sps_loc_align(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_init_host, int iters,
                  int min_corr, double tol_t, double tol_r, double *T_out_dev, int32_t *status_dev, double *trace_dev,
                  double *normal_dev, void *scratch_dev, void *stream) {
  if (!c || !n_dev || !T_init_host || !T_out_dev || !status_dev || !scratch_dev || cap < 0 || iters < 0 ||
      (cap > 0 && !pts_dev) || (iters > 0 && !trace_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (!c->rg.h.keys) return fail(SPS_ERR_INVALID, "sps_radius_grid_upload has not been called");
  if (cap > SPS_MAX_POINTS || iters > 10000) return fail(SPS_ERR_INVALID, "too many points or iterations");
  if (std::isnan(tol_t) || std::isnan(tol_r)) return fail(SPS_ERR_INVALID, "tolerances must not be NaN");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  LocPose T0;
  for (int i = 0; i < 16; ++i) T0.m[i] = T_init_host[i];
  const int nb = (int)loc_align_blocks(cap);
  double *partial = (double *)scratch_dev;
  int *done = (int *)(partial + (size_t)nb * LOC_TERMS);
  if (iters > 0) HIP_TRY(hipMemsetAsync(trace_dev, 0, (size_t)iters * 4 * sizeof(double), st));
  if (iters > 0 && normal_dev) HIP_TRY(hipMemsetAsync(normal_dev, 0, (size_t)iters * 28 * sizeof(double), st));
  hipLaunchKernelGGL(k_loc_init, dim3(1), dim3(64), 0, st, T0, T_out_dev, status_dev, done);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(k_loc_assoc, dim3(nb), dim3(256), 0, st, pts_dev, n_dev, (int)cap, c->rg, (const double *)T_out_dev,
                       (const int *)done, partial);
    hipLaunchKernelGGL(k_loc_solve, dim3(1), dim3(256), 0, st, (const double *)partial, n_dev, (int)cap, it, min_corr, tol_t,
                       tol_r, T0, T_out_dev, status_dev, done, trace_dev, normal_dev);
  }
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
