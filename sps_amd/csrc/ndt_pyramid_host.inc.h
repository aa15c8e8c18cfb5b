// ndt_pyramid_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_update_host.inc.h): the NDT
// localiser registering coarse to fine (ABI: the "NDT localiser, multi-resolution pyramid" section of include/sps_hip.h;
// kernels: ndt_pyramid_kernels.inc.h).  sps_ndt_pyramid_build allocates and synchronises, like sps_ndt_map_build, and
// leaves the context's single map (c->ndt, c->ndt_dyn) alone (ndt_pyramid_build_impl, which also builds the dynamic pyramid
// of ndt_pyramid_update_host.inc.h); sps_ndt_pyramid_align does neither: its scratch is the caller's.

namespace {
inline int64_t ndt_pyr_partial_bytes(int64_t cap) { return loc_align_blocks(cap) * LOC_TERMS * 8; }

// The pyramid of the context, static (cell_capacity == nullptr) or dynamic (level l has room for cell_capacity[l] cells, as
// the single dynamic map has).  Either replaces whatever pyramid the context had and leaves c->ndt and c->ndt_dyn alone.
// Allocates and synchronises.
int ndt_pyramid_build_impl(sps_ctx *c, int n_levels, const uint64_t *const *cell_keys_dev, const int32_t *const *cell_start_dev,
                           const int32_t *const *cell_pts_dev, const int64_t *n_cells, const double *resolution,
                           const double *map_xyz_dev, int64_t n_map, int min_points, double eig_ratio, double outlier_ratio,
                           const int64_t *cell_capacity, void *stream) {
  const bool dynamic = cell_capacity != nullptr;
  if (!c || !cell_keys_dev || !cell_start_dev || !cell_pts_dev || !n_cells || !resolution) return fail(SPS_ERR_INVALID, "bad arguments");
  if (n_levels < 1 || n_levels > NDT_PYR_MAX) return fail(SPS_ERR_INVALID, "n_levels must be in [1, %d]", NDT_PYR_MAX);
  NdtGauss gs[NDT_PYR_MAX];
  for (int l = 0; l < n_levels; ++l) {
    if (int e = ndt_map_check_args(c, cell_keys_dev[l], cell_start_dev[l], cell_pts_dev[l], map_xyz_dev, n_cells[l], n_map,
                                   resolution[l], min_points, eig_ratio, dynamic, dynamic ? cell_capacity[l] : 0))
      return e;
    if (l > 0 && !(resolution[l] < resolution[l - 1])) return fail(SPS_ERR_INVALID, "resolutions must be strictly decreasing");
    if (!ndt_gauss_fit(resolution[l], outlier_ratio, gs[l])) return SPS_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipDeviceSynchronize());
  for (void *p : c->ndt_pyr_allocs) (void)hipFree(p);
  c->ndt_pyr_allocs.clear();
  c->ndt_pyr = NdtPyramid{};
  NdtPyrLevel lv[NDT_PYR_MAX]{};
  NdtDyn dy[NDT_PYR_MAX]{};
  int32_t state0[NDT_PYR_MAX][4];   // read by copies in flight until the synchronisation below; a static map copies none
  for (int l = 0; l < n_levels; ++l) {
    if (int e = ndt_map_make(c->ndt_pyr_allocs, cell_keys_dev[l], cell_start_dev[l], cell_pts_dev[l], map_xyz_dev, n_cells[l], n_map,
                             resolution[l], min_points, eig_ratio, dynamic, dynamic ? cell_capacity[l] : 0, st, state0[l],
                             lv[l].m, dy[l]))
      return e;
    lv[l].gs = gs[l];
  }
  NdtPyrLevel *dev = nullptr;
  if (hipMalloc((void **)&dev, sizeof(lv)) != hipSuccess) return fail(SPS_ERR_NOMEM, "hipMalloc for the NDT pyramid failed");
  c->ndt_pyr_allocs.push_back(dev);
  HIP_TRY(hipMemcpyAsync(dev, lv, sizeof(lv), hipMemcpyHostToDevice, st));
  NdtDyn *dyn_dev = nullptr;
  if (dynamic) {
    if (hipMalloc((void **)&dyn_dev, sizeof(dy)) != hipSuccess) return fail(SPS_ERR_NOMEM, "hipMalloc for the NDT pyramid failed");
    c->ndt_pyr_allocs.push_back(dyn_dev);
    HIP_TRY(hipMemcpyAsync(dyn_dev, dy, sizeof(dy), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipStreamSynchronize(st));   // lv, dy and state0 are on this frame
  for (int l = 0; l < n_levels; ++l) c->ndt_pyr.lv[l] = lv[l], c->ndt_pyr.dyn[l] = dy[l];
  c->ndt_pyr.dev = dev;
  c->ndt_pyr.dynamic = dynamic;
  c->ndt_pyr.dyn_dev = dyn_dev;
  c->ndt_pyr.n_levels = n_levels;
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
  return ndt_pyramid_build_impl(c, n_levels, cell_keys_dev, cell_start_dev, cell_pts_dev, n_cells, resolution, map_xyz_dev, n_map,
                                min_points, eig_ratio, outlier_ratio, nullptr, stream);
}

int sps_ndt_pyramid_cells(sps_ctx *c, int level, uint64_t *key_out_dev, int32_t *count_out_dev, double *mean_out_dev,
                          double *icov_out_dev, int32_t *valid_out_dev) {
  if (!c) return fail(SPS_ERR_INVALID, "ctx is null");
  if (c->ndt_pyr.n_levels < 1) return fail(SPS_ERR_INVALID, "sps_ndt_pyramid_build has not been called");
  if (level < 0 || level >= c->ndt_pyr.n_levels) return fail(SPS_ERR_INVALID, "level must be in [0, %d)", c->ndt_pyr.n_levels);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  const NdtMap &m = c->ndt_pyr.lv[level].m;
  if (m.n_cells > 0)
    hipLaunchKernelGGL(k_ndt_cells_get, dim3((unsigned)((m.n_cells + 255) / 256)), dim3(256), 0, 0, m,
                       (unsigned long long *)key_out_dev, count_out_dev, mean_out_dev, icov_out_dev, valid_out_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return SPS_OK;
}

int sps_ndt_pyramid_align(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_init_host, int iters,
                          const int32_t *level_iters, int neighbours, int min_corr, double tol_t, double tol_r, double *T_out_dev,
                          int32_t *status_dev, double *trace_dev, double *normal_dev, int32_t *level_dev, void *scratch_dev,
                          void *stream) {
  if (!c || !n_dev || !T_init_host || !level_iters || !T_out_dev || !status_dev || !scratch_dev || cap < 0 || iters < 0 ||
      (cap > 0 && !pts_dev) || (iters > 0 && (!trace_dev || !level_dev)))
    return fail(SPS_ERR_INVALID, "bad arguments");
  const int L = c->ndt_pyr.n_levels;
  if (L < 1) return fail(SPS_ERR_INVALID, "sps_ndt_pyramid_build has not been called");
  if (int e = ndt_check_scan_limits(neighbours, cap, true, iters, tol_t, tol_r)) return e;
  NdtPyrCaps caps{};
  for (int l = 0; l < NDT_PYR_MAX; ++l) {
    caps.v[l] = l < L ? level_iters[l] : 1;
    if (caps.v[l] < 1) return fail(SPS_ERR_INVALID, "level_iters must be >= 1");
  }
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
    hipLaunchKernelGGL(k_ndt_pyr_assoc, dim3(nb), dim3(256), 0, st, pts_dev, n_dev, (int)cap, c->ndt_pyr.dev, L, neighbours,
                       (const double *)T_out_dev, (const int *)state, partial);
    hipLaunchKernelGGL(k_ndt_pyr_solve, dim3(1), dim3(256), 0, st, (const double *)partial, n_dev, (int)cap, it, L, caps, min_corr,
                       tol_t, tol_r, T0, T_out_dev, status_dev, state, trace_dev, normal_dev, level_dev);
  }
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
