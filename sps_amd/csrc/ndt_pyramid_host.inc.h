// ndt_pyramid_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_online_host.inc.h): the NDT
// localiser registering coarse to fine (ABI: the "NDT localiser, multi-resolution pyramid" section of include/sps_hip.h;
// kernels: ndt_pyramid_kernels.inc.h).  sps_ndt_pyramid_build allocates and synchronises, like sps_ndt_map_build, and
// leaves the context's single map alone (both are ndt_build_impl of ndt_host.inc.h, on the context's two slots; the online
// pyramid is in ndt_online_host.inc.h); sps_ndt_pyramid_align does neither: its scratch is the caller's.

namespace {
inline int64_t ndt_pyr_partial_bytes(int64_t cap) { return loc_align_blocks(cap) * LOC_TERMS * 8; }

// level_iters -> the caps of the L levels, by value for launch B (the levels past L get 1 and are never reached)
inline int ndt_pyr_caps(int L, const int32_t *level_iters, NdtPyrCaps &caps) {
  for (int l = 0; l < NDT_PYR_MAX; ++l) {
    caps.v[l] = l < L ? level_iters[l] : 1;
    if (caps.v[l] < 1) return fail(SPS_ERR_INVALID, "level_iters must be >= 1");
  }
  return SPS_OK;
}

// the coarse-to-fine alignment with the launches A and B of one scan (k_ndt_pyr_assoc / k_ndt_pyr_solve of NdtPoints:
// sps_ndt_pyramid_align; of NdtCells: sps_ndt_pyramid_align_d2d, whose elements are the levels' source records)
int ndt_pyramid_align_impl(NdtPyrAssocKernel assoc, NdtPyrSolveKernel solve, sps_ctx *c, const double *elems_dev,
                           const int32_t *n_dev, int64_t cap, const double *T_init_host, int iters, const int32_t *level_iters,
                           int neighbours, int min_corr, double tol_t, double tol_r, double *T_out_dev, int32_t *status_dev,
                           double *trace_dev, double *normal_dev, int32_t *level_dev, void *scratch_dev, void *stream) {
  if (!c || !n_dev || !T_init_host || !level_iters || !T_out_dev || !status_dev || !scratch_dev || cap < 0 || iters < 0 ||
      (cap > 0 && !elems_dev) || (iters > 0 && (!trace_dev || !level_dev)))
    return fail(SPS_ERR_INVALID, "bad arguments");
  const int L = c->ndt_pyr.n_levels;
  if (L < 1) return fail(SPS_ERR_INVALID, "sps_ndt_pyramid_build has not been called");
  if (int e = ndt_check_scan_limits(neighbours, cap, true, iters, tol_t, tol_r)) return e;
  NdtPyrCaps caps{};
  if (int e = ndt_pyr_caps(L, level_iters, caps)) return e;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  LocPose T0;
  for (int i = 0; i < 16; ++i) T0.m[i] = T_init_host[i];
  const int nb = (int)loc_align_blocks(cap);
  double *partial = (double *)scratch_dev;
  int *state = (int *)((char *)scratch_dev + ndt_pyr_partial_bytes(cap));
  const int init_blocks = std::min(64, std::max(1, (iters * 28 + 255) / 256));
  hipLaunchKernelGGL(k_ndt_pyr_init, dim3(init_blocks), dim3(256), 0, st, T0, iters, T_out_dev, status_dev, state, trace_dev,
                     normal_dev, level_dev);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(assoc, dim3(nb), dim3(256), 0, st, elems_dev, n_dev, (int)cap, c->ndt_pyr.dev, L, neighbours,
                       (const double *)T_out_dev, (const int *)state, partial);
    hipLaunchKernelGGL(solve, dim3(1), dim3(256), 0, st, (const double *)partial, n_dev, (int)cap, it, L, caps, min_corr,
                       tol_t, tol_r, T0, T_out_dev, status_dev, state, trace_dev, normal_dev, level_dev);
  }
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
}  // namespace

// the partial rows of k_ndt_pyr_solve, then the state words
int64_t sps_ndt_pyramid_align_scratch(int64_t cap) {
  if (cap < 0 || cap > SPS_MAX_POINTS) return -1;
  return ndt_pyr_partial_bytes(cap) + NDT_PYR_STATE * 4;
}

int sps_ndt_pyramid_build(sps_ctx *c, int n_levels, const uint64_t *const *cell_keys_dev, const int32_t *const *cell_start_dev,
                          const int32_t *const *cell_pts_dev, const int64_t *n_cells, const double *resolution,
                          const double *map_xyz_dev, int64_t n_map, int min_points, double eig_ratio, double outlier_ratio,
                          void *stream) {
  return ndt_build_impl(c, &sps_ctx::ndt_pyr, n_levels, cell_keys_dev, cell_start_dev, cell_pts_dev, n_cells, resolution,
                        map_xyz_dev, n_map, min_points, eig_ratio, &outlier_ratio, nullptr, stream);
}

int sps_ndt_pyramid_cells(sps_ctx *c, int level, uint64_t *key_out_dev, int32_t *count_out_dev, double *mean_out_dev,
                          double *icov_out_dev, int32_t *valid_out_dev) {
  return ndt_cells_impl(c, &sps_ctx::ndt_pyr, "sps_ndt_pyramid_build has not been called", level, key_out_dev, count_out_dev,
                        mean_out_dev, icov_out_dev, valid_out_dev);
}

int sps_ndt_pyramid_align(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_init_host, int iters,
                          const int32_t *level_iters, int neighbours, int min_corr, double tol_t, double tol_r, double *T_out_dev,
                          int32_t *status_dev, double *trace_dev, double *normal_dev, int32_t *level_dev, void *scratch_dev,
                          void *stream) {
  return ndt_pyramid_align_impl(k_ndt_pyr_assoc<NdtPoints>, k_ndt_pyr_solve<NdtPoints>, c, pts_dev, n_dev, cap, T_init_host, iters,
                                level_iters, neighbours, min_corr, tol_t, tol_r, T_out_dev, status_dev, trace_dev, normal_dev,
                                level_dev, scratch_dev, stream);
}
