// ndt_d2d_pyramid_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_pyramid_host.inc.h): the
// entry points of distribution-to-distribution NDT registered coarse to fine (ABI: the "NDT localiser, distribution to
// distribution, pyramid" section of include/sps_hip.h; kernels: ndt_d2d_pyramid_kernels.inc.h).  Neither call
// allocates or synchronises: the scratch is the caller's.  The scratch of the source build is ndt_src_layout's
// (ndt_d2d_host.inc.h) for n_levels levels, array-major.

int64_t sps_ndt_pyramid_source_scratch(int64_t cap, int n_levels) {
  if (cap < 0 || cap > SPS_NDT_UPDATE_MAX_POINTS || n_levels < 1 || n_levels > NDT_PYR_MAX) return -1;
  return (int64_t)ndt_src_layout(cap, n_levels, 1.0, nullptr, nullptr);
}

int sps_ndt_pyramid_source_build(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, int n_levels,
                                 const double *source_resolution, const int32_t *min_points, double eig_ratio, double *src_dev,
                                 int32_t *src_count_dev, int32_t *n_src_dev, void *scratch_dev, void *stream) {
  if (!c || !n_dev || !n_src_dev || !scratch_dev || !source_resolution || !min_points || cap < 0 ||
      (cap > 0 && (!pts_dev || !src_dev)))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (n_levels < 1 || n_levels > NDT_PYR_MAX) return fail(SPS_ERR_INVALID, "n_levels must be in [1, %d]", NDT_PYR_MAX);
  if (cap > SPS_NDT_UPDATE_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_NDT_UPDATE_MAX_POINTS);
  NdtPyrSrcParams p{};
  for (int l = 0; l < NDT_PYR_MAX; ++l) {
    p.resolution[l] = l < n_levels ? source_resolution[l] : 1.0;
    p.min_points[l] = l < n_levels ? min_points[l] : 0;
    if (!(p.resolution[l] > 0.0) || std::isinf(p.resolution[l]))
      return fail(SPS_ERR_INVALID, "source_resolution must be finite and > 0");
    if (p.min_points[l] < 0) return fail(SPS_ERR_INVALID, "min_points must be >= 0");
  }
  if (!(eig_ratio > 0.0) || !(eig_ratio <= 1.0)) return fail(SPS_ERR_INVALID, "eig_ratio must be in (0, 1]");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  NdtSrcLayout Y{};
  ndt_src_layout(cap, n_levels, 1.0, (char *)scratch_dev, &Y);
  LocPose I{};
  I.m[0] = I.m[5] = I.m[10] = I.m[15] = 1.0;
  const unsigned L = (unsigned)n_levels;
  const unsigned nbp = (unsigned)((cap + 255) / 256 > 0 ? (cap + 255) / 256 : 1);
  const unsigned nbs = (unsigned)std::min<int64_t>(std::max<int64_t>(cap / 4, 1), 2048);
  HIP_TRY(hipMemsetAsync(Y.ff, 0xFF, Y.ff_bytes, st));
  HIP_TRY(hipMemsetAsync(Y.sf, 0x7F, Y.sf_bytes, st));
  HIP_TRY(hipMemsetAsync(Y.zero, 0, Y.zero_bytes, st));
  HIP_TRY(hipMemsetAsync(n_src_dev, 0, (size_t)L * 2 * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_ndt_pyr_src_lookup, dim3(nbp, L), dim3(256), 0, st, pts_dev, n_dev, (int)cap, I, Y.m, Y.s, Y.w, p);
  hipLaunchKernelGGL(k_ndt_pyr_src_found, dim3(1, L), dim3(NDT_UPD_BLOCK), 0, st, n_dev, (int)cap, Y.d, Y.s, Y.w, Y.info);
  hipLaunchKernelGGL(k_ndt_pyr_src_resolve, dim3(nbp, L), dim3(256), 0, st, n_dev, (int)cap, Y.m, Y.d, Y.s, Y.w, p);
  hipLaunchKernelGGL(k_ndt_pyr_src_offsets, dim3(1, L), dim3(NDT_UPD_BLOCK), 0, st, n_dev, (int)cap, Y.d, Y.s, Y.w, Y.info);
  hipLaunchKernelGGL(k_ndt_pyr_src_fill, dim3(nbp, L), dim3(256), 0, st, n_dev, (int)cap, Y.d, Y.s, Y.w);
  hipLaunchKernelGGL(k_ndt_pyr_src_stats, dim3(nbs, L), dim3(64), 0, st, n_dev, (int)cap, Y.d, Y.s, Y.w);
  hipLaunchKernelGGL(k_ndt_pyr_src_records, dim3(nbp, L), dim3(256), 0, st, n_dev, (int)cap, p, eig_ratio, Y.s, Y.w, src_dev,
                     src_count_dev, n_src_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

// the partial rows of launch B (one per 32 sources), then the state words: sps_ndt_pyramid_align_scratch's layout
int64_t sps_ndt_pyramid_align_d2d_scratch(int64_t cap_src) {
  if (cap_src < 0 || cap_src > SPS_MAX_POINTS) return -1;
  return ndt_pyr_partial_bytes(cap_src) + NDT_PYR_STATE * 4;
}

int sps_ndt_pyramid_align_d2d(sps_ctx *c, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src,
                              const double *T_init_host, int iters, const int32_t *level_iters, int neighbours, int min_corr,
                              double tol_t, double tol_r, double *T_out_dev, int32_t *status_dev, double *trace_dev,
                              double *normal_dev, int32_t *level_dev, void *scratch_dev, void *stream) {
  if (!c || !n_src_dev || !T_init_host || !level_iters || !T_out_dev || !status_dev || !scratch_dev || cap_src < 0 || iters < 0 ||
      (cap_src > 0 && !src_dev) || (iters > 0 && (!trace_dev || !level_dev)))
    return fail(SPS_ERR_INVALID, "bad arguments");
  const int L = c->ndt_pyr.n_levels;
  if (L < 1) return fail(SPS_ERR_INVALID, "sps_ndt_pyramid_build has not been called");
  if (int e = ndt_check_scan_limits(neighbours, cap_src, true, iters, tol_t, tol_r)) return e;
  NdtPyrCaps caps{};
  for (int l = 0; l < NDT_PYR_MAX; ++l) {
    caps.v[l] = l < L ? level_iters[l] : 1;
    if (caps.v[l] < 1) return fail(SPS_ERR_INVALID, "level_iters must be >= 1");
  }
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  LocPose T0;
  for (int i = 0; i < 16; ++i) T0.m[i] = T_init_host[i];
  const int nb = (int)loc_align_blocks(cap_src);
  double *partial = (double *)scratch_dev;
  int *state = (int *)((char *)scratch_dev + ndt_pyr_partial_bytes(cap_src));
  const int init_blocks = std::min(64, std::max(1, (iters * 28 + 255) / 256));
  hipLaunchKernelGGL(k_ndt_pyr_init, dim3(init_blocks), dim3(256), 0, st, T0, iters, T_out_dev, status_dev, state, trace_dev,
                     normal_dev, level_dev);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(k_ndt_d2d_pyr_assoc, dim3(nb), dim3(256), 0, st, src_dev, n_src_dev, (int)cap_src, c->ndt_pyr.dev, L,
                       neighbours, (const double *)T_out_dev, (const int *)state, partial);
    hipLaunchKernelGGL(k_ndt_d2d_pyr_solve, dim3(1), dim3(256), 0, st, (const double *)partial, n_src_dev, (int)cap_src, it, L,
                       caps, min_corr, tol_t, tol_r, T0, T_out_dev, status_dev, state, trace_dev, normal_dev, level_dev);
  }
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
