// ndt_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block): the entry points of the NDT localiser
// (ABI: the "NDT localiser" section of include/sps_hip.h; kernels: ndt_kernels.inc.h).  sps_ndt_map_build allocates and
// synchronises, like sps_radius_grid_upload; sps_ndt_align does neither: its scratch is the caller's.  The single map of a
// context is a pyramid of one level (sps_ctx::ndt_map), so three helpers here serve the single map and the pyramid alike
// and the later NDT files too: ndt_build_impl (every build: static or dynamic, one level or several), ndt_cells_impl (both
// cell getters) and ndt_check_scan_args (the checks that the alignment, the batch and the pose score share).  What is
// registered, the thinned points or the scan's own cells, is a type (NdtPoints, NdtCells) that launch A's body is a template
// over: ndt_align_batch_impl, ndt_score_poses_impl and ndt_pyramid_align_impl of the later files take the scan's kernel
// instantiation as an argument, and the entry points of ndt_d2d_host.inc.h hand them NdtCells'.  The single alignment's two
// entry points keep a host body each (sps_ndt_align here, sps_ndt_align_d2d there; see k_ndt_assoc).

namespace {
// the Gaussian fit of the mixture (Magnusson 2009, eq. 6.8; PCL's gauss_d1_ / gauss_d2_), in float64 on the host; false
// (and the error text set) where outlier_ratio and the resolution give none
inline bool ndt_gauss_fit(double res, double outlier_ratio, NdtGauss &gs) {
  if (!(outlier_ratio > 0.0) || !(outlier_ratio < 1.0)) return fail(SPS_ERR_INVALID, "outlier_ratio must be in (0, 1)"), false;
  const double c1 = 10.0 * (1.0 - outlier_ratio), c2 = outlier_ratio / (res * res * res);
  const double d3 = -std::log(c2);
  const double d1 = -std::log(c1 + c2) - d3;
  const double d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / d1);
  if (!std::isfinite(d1) || !std::isfinite(d2) || !(d1 < 0.0) || !(d2 > 0.0))
    return fail(SPS_ERR_INVALID, "outlier_ratio and resolution give no usable Gaussian fit"), false;
  gs = NdtGauss{-d1, d2};
  return true;
}
// what sps_ndt_align, sps_ndt_align_batch and sps_ndt_score_poses ask alike of the context's map and of the scan, and the
// Gaussian fit.  aligns: the call iterates, so it also has an iteration limit and tolerances (sps_ndt_score_poses has
// neither, and its own text for the point limit); the checks stay in the order every entry point always made them
// (the part that does not look at a map is ndt_check_scan_limits: sps_ndt_pyramid_align, whose Gaussian fits were made
// by its build, asks the same of its scan)
inline int ndt_check_scan_limits(int neighbours, int64_t cap, bool aligns, int iters, double tol_t, double tol_r) {
  if (neighbours != 1 && neighbours != 7) return fail(SPS_ERR_INVALID, "neighbours must be 1 or 7");
  if (cap > SPS_MAX_POINTS || (aligns && iters > 10000))
    return aligns ? fail(SPS_ERR_INVALID, "too many points or iterations")
                  : fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_MAX_POINTS);
  if (aligns && (std::isnan(tol_t) || std::isnan(tol_r))) return fail(SPS_ERR_INVALID, "tolerances must not be NaN");
  return SPS_OK;
}
inline int ndt_check_scan_args(const sps_ctx *c, int neighbours, int64_t cap, double outlier_ratio, NdtGauss &gs, bool aligns,
                               int iters = 0, double tol_t = 0.0, double tol_r = 0.0) {
  if (c->ndt_map.n_levels < 1) return fail(SPS_ERR_INVALID, "sps_ndt_map_build has not been called");
  if (int e = ndt_check_scan_limits(neighbours, cap, aligns, iters, tol_t, tol_r)) return e;
  return ndt_gauss_fit(c->ndt_map.lv[0].m.resolution, outlier_ratio, gs) ? SPS_OK : SPS_ERR_INVALID;
}

inline int64_t ndt_hash_slots(int64_t cells) { return next_pow2(2 * (cells < 512 ? 512 : cells)); }
inline size_t ndt_upd_align(size_t v) { return (v + 255) & ~(size_t)255; }   // of the arrays cut from a caller's scratch

// what every map build asks of its arguments (cell_capacity is read for a dynamic map only)
inline int ndt_map_check_args(const sps_ctx *c, const uint64_t *cell_keys_dev, const int32_t *cell_start_dev,
                              const int32_t *cell_pts_dev, const double *map_xyz_dev, int64_t n_cells, int64_t n_map,
                              double resolution, int min_points, double eig_ratio, bool dynamic, int64_t cell_capacity) {
  if (!c || n_cells < 0 || n_map < 0 || n_cells > n_map) return fail(SPS_ERR_INVALID, "bad arguments");
  if (!(resolution > 0.0) || std::isinf(resolution)) return fail(SPS_ERR_INVALID, "resolution must be finite and > 0");
  if (!(eig_ratio > 0.0) || !(eig_ratio <= 1.0)) return fail(SPS_ERR_INVALID, "eig_ratio must be in (0, 1]");
  if (min_points < 0) return fail(SPS_ERR_INVALID, "min_points must be >= 0");
  if (n_map > 0 && (!cell_keys_dev || !cell_start_dev || !cell_pts_dev || !map_xyz_dev)) return fail(SPS_ERR_INVALID, "null argument");
  if (n_map >= (1ll << 31) || n_cells >= (1ll << 30)) return fail(SPS_ERR_INVALID, "map too large");
  if (dynamic && (cell_capacity < 1 || cell_capacity < n_cells)) return fail(SPS_ERR_INVALID, "cell_capacity must be >= max(n_cells, 1)");
  if (dynamic && cell_capacity >= (1ll << 30)) return fail(SPS_ERR_INVALID, "cell_capacity too large");
  return SPS_OK;
}

// One cell map from checked arguments, its memory added to `allocs`: the hash, the records, the counts and the keys (and
// for a dynamic map the moments S, the update's per-cell state and the carving's three counters), filled on stream st.
// Does not synchronise: state0 (the caller's, four words) is read by a copy still in flight on return.  m and d are
// written only on success.
int ndt_map_make(std::vector<void *> &allocs, const uint64_t *cell_keys_dev, const int32_t *cell_start_dev,
                 const int32_t *cell_pts_dev, const double *map_xyz_dev, int64_t n_cells, int64_t n_map, double resolution,
                 int min_points, double eig_ratio, bool dynamic, int64_t cell_capacity, hipStream_t st, int32_t *state0,
                 NdtMap &m_out, NdtDyn &d_out) {
  bool nomem = false;
  auto alloc = [&](size_t bytes) -> void * {
    void *p = nullptr;
    if (nomem || hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nomem = true, nullptr;
    allocs.push_back(p);
    return p;
  };
  const size_t C = (size_t)(dynamic ? cell_capacity : n_cells);
  const int64_t hcap = ndt_hash_slots((int64_t)C);
  NdtMap m{};
  NdtDyn d{};
  m.h.keys = (uint64_t *)alloc((size_t)hcap * 8);
  m.h.first = nullptr;
  m.h.rank = (int *)alloc((size_t)hcap * 4);
  m.h.mask = (uint32_t)(hcap - 1);
  m.rec = d.rec = (double *)alloc(C * NDT_REC * 8);
  m.count = d.count = (int *)alloc(C * 4);
  m.keys = d.keys = (uint64_t *)alloc(C * 8);
  m.n_cells = (int)C;
  m.resolution = resolution;
  if (dynamic) {
    d.capacity = (int)cell_capacity, d.min_points = min_points, d.eig_ratio = eig_ratio;
    d.S = (double *)alloc(C * 6 * 8), d.bcnt = (int *)alloc(C * 4), d.lead = (int *)alloc(C * 4);
    d.cstart = (int *)alloc(C * 4), d.state = (int *)alloc(16);
    d.pass = (int *)alloc(C * 4), d.hit = (int *)alloc(C * 4), d.miss = (int *)alloc(C * 4);
  }
  if (nomem) return fail(SPS_ERR_NOMEM, "hipMalloc for the NDT map failed");
  HIP_TRY(hipMemsetAsync(m.h.keys, 0xFF, (size_t)hcap * 8, st));
  HIP_TRY(hipMemsetAsync(m.h.rank, 0xFF, (size_t)hcap * 4, st));
  state0[0] = (int32_t)n_cells, state0[1] = state0[2] = state0[3] = 0;
  if (dynamic) {   // the rest values of the cells that the updates will found
    HIP_TRY(hipMemsetAsync(d.rec, 0, C * NDT_REC * 8, st));
    HIP_TRY(hipMemsetAsync(d.count, 0, C * 4, st));
    HIP_TRY(hipMemsetAsync(d.keys, 0xFF, C * 8, st));
    HIP_TRY(hipMemsetAsync(d.S, 0, C * 6 * 8, st));
    HIP_TRY(hipMemsetAsync(d.bcnt, 0, C * 4, st));
    HIP_TRY(hipMemsetAsync(d.lead, 0x7F, C * 4, st));
    HIP_TRY(hipMemsetAsync(d.cstart, 0, C * 4, st));
    HIP_TRY(hipMemsetAsync(d.pass, 0, C * 4, st));
    HIP_TRY(hipMemsetAsync(d.hit, 0, C * 4, st));
    HIP_TRY(hipMemsetAsync(d.miss, 0, C * 4, st));
    HIP_TRY(hipMemcpyAsync(d.state, state0, 4 * sizeof(int32_t), hipMemcpyHostToDevice, st));
  }
  if (n_cells > 0) {
    const unsigned nb = (unsigned)((n_cells + 255) / 256);
    HIP_TRY(hipMemcpyAsync(d.keys, cell_keys_dev, (size_t)n_cells * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_radius_cells_insert, dim3(nb), dim3(256), 0, st, (const unsigned long long *)cell_keys_dev, (int)n_cells, m.h);
    hipLaunchKernelGGL(k_ndt_cells, dim3(nb), dim3(256), 0, st, (const int *)cell_start_dev, (const int *)cell_pts_dev, map_xyz_dev,
                       (int)n_cells, (int)n_map, min_points, eig_ratio, d.rec, d.count, d.S);
  }
  HIP_TRY(hipGetLastError());
  m_out = m, d_out = d;
  return SPS_OK;
}

// One of the two pyramids of the context (`slot`: the single map, n_levels == 1, or the pyramid), static (cell_capacity ==
// nullptr: level l has room for the n_cells[l] of the build) or dynamic (room for cell_capacity[l] cells, their moments S,
// the update's per-cell state and the carve's counters beside the records).  outlier_ratio: of the levels' Gaussian fits;
// nullptr for the single map, whose alignments take the ratio per call, so its gs stays zero and nothing reads it.  Replaces
// whatever that slot held and leaves the other slot alone.  Allocates and synchronises.
int ndt_build_impl(sps_ctx *c, NdtPyramid sps_ctx::*slot, int n_levels, const uint64_t *const *cell_keys_dev,
                   const int32_t *const *cell_start_dev, const int32_t *const *cell_pts_dev, const int64_t *n_cells,
                   const double *resolution, const double *map_xyz_dev, int64_t n_map, int min_points, double eig_ratio,
                   const double *outlier_ratio, const int64_t *cell_capacity, void *stream) {
  const bool dynamic = cell_capacity != nullptr;
  if (!c || !cell_keys_dev || !cell_start_dev || !cell_pts_dev || !n_cells || !resolution) return fail(SPS_ERR_INVALID, "bad arguments");
  if (n_levels < 1 || n_levels > NDT_PYR_MAX) return fail(SPS_ERR_INVALID, "n_levels must be in [1, %d]", NDT_PYR_MAX);
  NdtGauss gs[NDT_PYR_MAX]{};
  for (int l = 0; l < n_levels; ++l) {
    if (int e = ndt_map_check_args(c, cell_keys_dev[l], cell_start_dev[l], cell_pts_dev[l], map_xyz_dev, n_cells[l], n_map,
                                   resolution[l], min_points, eig_ratio, dynamic, dynamic ? cell_capacity[l] : 0))
      return e;
    if (l > 0 && !(resolution[l] < resolution[l - 1])) return fail(SPS_ERR_INVALID, "resolutions must be strictly decreasing");
    if (outlier_ratio && !ndt_gauss_fit(resolution[l], *outlier_ratio, gs[l])) return SPS_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipDeviceSynchronize());
  NdtPyramid &py = c->*slot;
  for (void *p : py.allocs) (void)hipFree(p);
  py = NdtPyramid{};
  NdtPyrLevel lv[NDT_PYR_MAX]{};
  NdtDyn dy[NDT_PYR_MAX]{};
  int32_t state0[NDT_PYR_MAX][4];   // read by copies in flight until the synchronisation below; a static map copies none
  for (int l = 0; l < n_levels; ++l) {
    if (int e = ndt_map_make(py.allocs, cell_keys_dev[l], cell_start_dev[l], cell_pts_dev[l], map_xyz_dev, n_cells[l], n_map,
                             resolution[l], min_points, eig_ratio, dynamic, dynamic ? cell_capacity[l] : 0, st, state0[l],
                             lv[l].m, dy[l]))
      return e;
    lv[l].gs = gs[l];
  }
  NdtPyrLevel *dev = nullptr;
  if (hipMalloc((void **)&dev, sizeof(lv)) != hipSuccess) return fail(SPS_ERR_NOMEM, "hipMalloc for the NDT pyramid failed");
  py.allocs.push_back(dev);
  HIP_TRY(hipMemcpyAsync(dev, lv, sizeof(lv), hipMemcpyHostToDevice, st));
  NdtDyn *dyn_dev = nullptr;
  if (dynamic) {
    if (hipMalloc((void **)&dyn_dev, sizeof(dy)) != hipSuccess) return fail(SPS_ERR_NOMEM, "hipMalloc for the NDT pyramid failed");
    py.allocs.push_back(dyn_dev);
    HIP_TRY(hipMemcpyAsync(dyn_dev, dy, sizeof(dy), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipStreamSynchronize(st));   // lv, dy and state0 are on this frame
  for (int l = 0; l < n_levels; ++l) py.lv[l] = lv[l], py.dyn[l] = dy[l];
  py.dev = dev;
  py.dynamic = dynamic;
  py.dyn_dev = dyn_dev;
  py.n_levels = n_levels;
  return SPS_OK;
}

// the records of level `level` of a pyramid; not_built: the error text of a slot that holds none
int ndt_cells_impl(sps_ctx *c, NdtPyramid sps_ctx::*slot, const char *not_built, int level, uint64_t *key_out_dev,
                   int32_t *count_out_dev, double *mean_out_dev, double *icov_out_dev, int32_t *valid_out_dev) {
  if (!c) return fail(SPS_ERR_INVALID, "ctx is null");
  const NdtPyramid &py = c->*slot;
  if (py.n_levels < 1) return fail(SPS_ERR_INVALID, "%s", not_built);
  if (level < 0 || level >= py.n_levels) return fail(SPS_ERR_INVALID, "level must be in [0, %d)", py.n_levels);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  const NdtMap &m = py.lv[level].m;
  if (m.n_cells > 0)
    hipLaunchKernelGGL(k_ndt_cells_get, dim3((unsigned)((m.n_cells + 255) / 256)), dim3(256), 0, 0, m,
                       (unsigned long long *)key_out_dev, count_out_dev, mean_out_dev, icov_out_dev, valid_out_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return SPS_OK;
}
}  // namespace

int64_t sps_ndt_align_scratch(int64_t cap) { return sps_loc_align_scratch(cap); }   // the partial rows of k_loc_solve

int sps_ndt_map_build(sps_ctx *c, const uint64_t *cell_keys_dev, const int32_t *cell_start_dev, const int32_t *cell_pts_dev,
                      const double *map_xyz_dev, int64_t n_cells, int64_t n_map, double resolution, int min_points,
                      double eig_ratio, void *stream) {
  return ndt_build_impl(c, &sps_ctx::ndt_map, 1, &cell_keys_dev, &cell_start_dev, &cell_pts_dev, &n_cells, &resolution,
                        map_xyz_dev, n_map, min_points, eig_ratio, nullptr, nullptr, stream);
}

int sps_ndt_map_cells(sps_ctx *c, uint64_t *key_out_dev, int32_t *count_out_dev, double *mean_out_dev, double *icov_out_dev,
                      int32_t *valid_out_dev) {
  return ndt_cells_impl(c, &sps_ctx::ndt_map, "sps_ndt_map_build has not been called", 0, key_out_dev, count_out_dev,
                        mean_out_dev, icov_out_dev, valid_out_dev);
}

int sps_ndt_align(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_init_host, int iters,
                  int neighbours, int min_corr, double outlier_ratio, double tol_t, double tol_r, double *T_out_dev,
                  int32_t *status_dev, double *trace_dev, double *normal_dev, void *scratch_dev, void *stream) {
  if (!c || !n_dev || !T_init_host || !T_out_dev || !status_dev || !scratch_dev || cap < 0 || iters < 0 ||
      (cap > 0 && !pts_dev) || (iters > 0 && !trace_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  NdtGauss gs;
  if (int e = ndt_check_scan_args(c, neighbours, cap, outlier_ratio, gs, true, iters, tol_t, tol_r)) return e;
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
    hipLaunchKernelGGL(k_ndt_assoc, dim3(nb), dim3(256), 0, st, pts_dev, n_dev, (int)cap, c->ndt_map.lv[0].m, gs, neighbours,
                       (const double *)T_out_dev, (const int *)done, partial);
    hipLaunchKernelGGL(k_loc_solve, dim3(1), dim3(256), 0, st, (const double *)partial, n_dev, (int)cap, it, min_corr, tol_t,
                       tol_r, T0, T_out_dev, status_dev, done, trace_dev, normal_dev);
  }
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
