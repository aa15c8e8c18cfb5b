// ndt_online_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_search_host.inc.h): the
// online NDT maps (ABI: the "NDT localiser, online map", "... online map: free-space carving" and "... online pyramid"
// sections of include/sps_hip.h; kernels: ndt_online_kernels.inc.h).  The single map of a context
// is a pyramid of one level, so there is one implementation of the update, the carve and their getters: it takes the
// slot of the context and the slot's error text, and the sps_ndt_map_* and sps_ndt_pyramid_* entry points below are its
// calls.  The dynamic builds are ndt_build_impl (ndt_host.inc.h) with a cell capacity per level: they allocate and
// synchronise.  The update and the carve do neither, and what they issue can be read off below: seven launches and two
// memsets, and three launches, whatever the number of levels and the data.

namespace {
const char *const NDT_MAP_NOT_DYNAMIC = "the map of this context is not dynamic (sps_ndt_map_build_dynamic)";
const char *const NDT_PYR_NOT_DYNAMIC = "the pyramid of this context is not dynamic (sps_ndt_pyramid_build_dynamic)";

// The caller's scratch cut into its arrays, array-major: every per-level array holds the L levels back to back, so the
// hash keys of all levels are one range and their `first` arrays another (one memset each).  *s is level 0's view, *w what
// turns it into level l's (ndt_pyr_upd_slice).  base == nullptr: only the size is wanted.
inline size_t ndt_pyr_upd_layout(int64_t cap, int L, char *base, NdtUpdScratch *s, NdtPyrUpdStride *w) {
  const size_t n = (size_t)(cap < 1 ? 1 : cap), hs = (size_t)ndt_hash_slots(cap), l = (size_t)L;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char *p = base ? base + at : nullptr;
    at += ndt_upd_align(bytes);
    return p;
  };
  char *q = take(n * 3 * 8), *bstat = take(l * n * 10 * 8), *hkeys = take(l * hs * 8), *cell_of = take(l * n * 4),
       *slot_of = take(l * n * 4), *list = take(l * n * 4), *tcell = take(l * n * 4), *hfirst = take(l * hs * 4),
       *hrank = take(l * hs * 4), *nt = take(l * 4);
  if (s) {
    s->q = (double *)q, s->bstat = (double *)bstat, s->cell_of = (int *)cell_of, s->slot_of = (int *)slot_of;
    s->list = (int *)list, s->tcell = (int *)tcell, s->n_touched = (int *)nt;
    s->h.keys = (uint64_t *)hkeys, s->h.first = (int *)hfirst, s->h.rank = (int *)hrank, s->h.mask = (uint32_t)(hs - 1);
  }
  if (w) w->n = (int)n, w->hs = (int)hs;
  return at;
}

// the slot holds a dynamic pyramid, or the error text is set
inline int ndt_check_dynamic(const NdtPyramid &py, const char *not_dynamic) {
  if (py.n_levels < 1 || !py.dynamic || !py.dyn_dev) return fail(SPS_ERR_INVALID, "%s", not_dynamic);
  return SPS_OK;
}

// info_dev: int32[n_levels][4]
int ndt_update_impl(sps_ctx *c, NdtPyramid sps_ctx::*slot, const char *not_dynamic, const double *pts_dev, const int32_t *n_dev,
                    int64_t cap, const double *T_host, const double *T_dev, const int32_t *gate_dev, int max_cell_points,
                    int32_t *info_dev, void *scratch_dev, void *stream) {
  if (!c || !n_dev || !info_dev || !scratch_dev || cap < 0 || (cap > 0 && !pts_dev) || (!T_host && !T_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  const NdtPyramid &py = c->*slot;
  if (int e = ndt_check_dynamic(py, not_dynamic)) return e;
  if (cap > SPS_NDT_UPDATE_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_NDT_UPDATE_MAX_POINTS);
  if (max_cell_points < 0) return fail(SPS_ERR_INVALID, "max_cell_points must be >= 0");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  LocPose Th{};
  if (T_host)
    for (int i = 0; i < 16; ++i) Th.m[i] = T_host[i];
  const unsigned L = (unsigned)py.n_levels;
  NdtUpdScratch s{};
  NdtPyrUpdStride w{};
  ndt_pyr_upd_layout(cap, (int)L, (char *)scratch_dev, &s, &w);
  const NdtPyrLevel *lv = py.dev;
  const NdtDyn *dy = py.dyn_dev;
  const unsigned nbp = (unsigned)((cap + 255) / 256 > 0 ? (cap + 255) / 256 : 1);
  const unsigned nbs = (unsigned)std::min<int64_t>(std::max<int64_t>(cap / 4, 1), 2048);
  // the levels' update hashes start empty whatever the gate says: they are scratch.  Two memsets cover all levels.
  HIP_TRY(hipMemsetAsync(s.h.keys, 0xFF, (size_t)L * (size_t)w.hs * 8, st));
  HIP_TRY(hipMemsetAsync(s.h.first, 0x7F, (size_t)L * (size_t)w.hs * 4, st));
  hipLaunchKernelGGL(k_ndt_upd_lookup, dim3(nbp, L), dim3(256), 0, st, pts_dev, n_dev, (int)cap, Th, T_dev, gate_dev, lv, s, w);
  hipLaunchKernelGGL(k_ndt_upd_found, dim3(1, L), dim3(NDT_UPD_BLOCK), 0, st, n_dev, (int)cap, gate_dev, dy, s, w, info_dev);
  hipLaunchKernelGGL(k_ndt_upd_resolve, dim3(nbp, L), dim3(256), 0, st, n_dev, (int)cap, gate_dev, lv, dy, s, w);
  hipLaunchKernelGGL(k_ndt_upd_offsets, dim3(1, L), dim3(NDT_UPD_BLOCK), 0, st, n_dev, (int)cap, gate_dev, dy, s, w, info_dev);
  hipLaunchKernelGGL(k_ndt_upd_fill, dim3(nbp, L), dim3(256), 0, st, n_dev, (int)cap, gate_dev, dy, s, w);
  hipLaunchKernelGGL(k_ndt_upd_stats, dim3(nbs, L), dim3(64), 0, st, n_dev, (int)cap, gate_dev, dy, s, w);
  hipLaunchKernelGGL(k_ndt_upd_merge, dim3(nbp, L), dim3(256), 0, st, n_dev, (int)cap, gate_dev, max_cell_points, dy, s, w);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

// end_margin: double[n_levels]; info_dev: int32[n_levels][4].  The carve's three per-cell arrays belong to the dynamic map
// (ndt_map_make, ndt_host.inc.h): it needs no scratch of the caller's.
int ndt_carve_impl(sps_ctx *c, NdtPyramid sps_ctx::*slot, const char *not_dynamic, const double *pts_dev, const int32_t *n_dev,
                   int64_t cap, const double *T_host, const double *T_dev, const int32_t *gate_dev, const double *end_margin,
                   double through_sigma, int min_pass, int miss_frames, int max_steps, int32_t *info_dev, void *stream) {
  if (!c || !n_dev || !info_dev || !end_margin || cap < 0 || (cap > 0 && !pts_dev) || (!T_host && !T_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  const NdtPyramid &py = c->*slot;
  if (int e = ndt_check_dynamic(py, not_dynamic)) return e;
  if (cap > SPS_NDT_UPDATE_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_NDT_UPDATE_MAX_POINTS);
  const int L = py.n_levels;
  NdtPyrMargins em{};
  int cmax = 1;
  for (int l = 0; l < L; ++l) {
    if (!(end_margin[l] >= 0.0) || std::isinf(end_margin[l])) return fail(SPS_ERR_INVALID, "end_margin must be finite and >= 0");
    em.v[l] = end_margin[l];
    cmax = std::max(cmax, py.dyn[l].capacity);
  }
  if (!(through_sigma > 0.0) || std::isinf(through_sigma)) return fail(SPS_ERR_INVALID, "through_sigma must be finite and > 0");
  if (min_pass < 1 || miss_frames < 1) return fail(SPS_ERR_INVALID, "min_pass and miss_frames must be >= 1");
  if (max_steps < 1 || max_steps > 4096) return fail(SPS_ERR_INVALID, "max_steps must be in [1, 4096]");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  LocPose Th{};
  if (T_host)
    for (int i = 0; i < 16; ++i) Th.m[i] = T_host[i];
  const NdtPyrLevel *lv = py.dev;
  const NdtDyn *dy = py.dyn_dev;
  const NdtCarveParams p{0.0, through_sigma * through_sigma, min_pass, miss_frames, max_steps};   // end_margin: per level, em
  const unsigned nbp = (unsigned)((cap + 255) / 256 > 0 ? (cap + 255) / 256 : 1);
  const unsigned nbc = (unsigned)((cmax + 255) / 256);   // the largest level's; a smaller level's surplus threads return
  hipLaunchKernelGGL(k_ndt_carve_begin, dim3(nbc, (unsigned)L), dim3(256), 0, st, gate_dev, dy, info_dev);
  hipLaunchKernelGGL(k_ndt_carve_rays, dim3(nbp, (unsigned)L), dim3(256), 0, st, pts_dev, n_dev, (int)cap, Th, T_dev, gate_dev, lv, dy,
                     p, em, info_dev);
  hipLaunchKernelGGL(k_ndt_carve_decide, dim3(nbc, (unsigned)L), dim3(256), 0, st, gate_dev, dy, p, info_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

// the checks the two getters of a level share, then the device at rest; d_out: the level's state
int ndt_level_at_rest(sps_ctx *c, NdtPyramid sps_ctx::*slot, const char *not_dynamic, int level, const NdtDyn *&d_out) {
  const NdtPyramid &py = c->*slot;
  if (int e = ndt_check_dynamic(py, not_dynamic)) return e;
  if (level < 0 || level >= py.n_levels) return fail(SPS_ERR_INVALID, "level must be in [0, %d)", py.n_levels);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  d_out = &py.dyn[level];
  return SPS_OK;
}

int ndt_info_impl(sps_ctx *c, NdtPyramid sps_ctx::*slot, const char *not_dynamic, int level, int64_t *out_host) {
  if (!c || !out_host) return fail(SPS_ERR_INVALID, "bad arguments");
  const NdtDyn *d = nullptr;
  if (int e = ndt_level_at_rest(c, slot, not_dynamic, level, d)) return e;
  int32_t st[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpy(st, d->state, sizeof(st), hipMemcpyDeviceToHost));
  out_host[0] = st[0], out_host[1] = d->capacity, out_host[2] = st[1], out_host[3] = 0;
  return SPS_OK;
}

int ndt_carve_cells_impl(sps_ctx *c, NdtPyramid sps_ctx::*slot, const char *not_dynamic, int level, int32_t *pass_out_dev,
                         int32_t *hit_out_dev, int32_t *miss_out_dev) {
  if (!c) return fail(SPS_ERR_INVALID, "ctx is null");
  const NdtDyn *d = nullptr;
  if (int e = ndt_level_at_rest(c, slot, not_dynamic, level, d)) return e;
  const size_t bytes = (size_t)d->capacity * sizeof(int32_t);
  if (pass_out_dev) HIP_TRY(hipMemcpy(pass_out_dev, d->pass, bytes, hipMemcpyDeviceToDevice));
  if (hit_out_dev) HIP_TRY(hipMemcpy(hit_out_dev, d->hit, bytes, hipMemcpyDeviceToDevice));
  if (miss_out_dev) HIP_TRY(hipMemcpy(miss_out_dev, d->miss, bytes, hipMemcpyDeviceToDevice));
  HIP_TRY(hipDeviceSynchronize());
  return SPS_OK;
}

inline bool ndt_online_cap_ok(int64_t cap) { return cap >= 0 && cap <= SPS_NDT_UPDATE_MAX_POINTS; }
}  // namespace

// ---- the single map: a pyramid of one level ------------------------------------------------------------------------------
int sps_ndt_map_build_dynamic(sps_ctx *c, const uint64_t *cell_keys_dev, const int32_t *cell_start_dev,
                              const int32_t *cell_pts_dev, const double *map_xyz_dev, int64_t n_cells, int64_t n_map,
                              double resolution, int min_points, double eig_ratio, int64_t cell_capacity, void *stream) {
  return ndt_build_impl(c, &sps_ctx::ndt_map, 1, &cell_keys_dev, &cell_start_dev, &cell_pts_dev, &n_cells, &resolution,
                        map_xyz_dev, n_map, min_points, eig_ratio, nullptr, &cell_capacity, stream);
}

int64_t sps_ndt_map_update_scratch(int64_t cap) { return sps_ndt_pyramid_update_scratch(cap, 1); }

int sps_ndt_map_update(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                       const double *T_dev, const int32_t *gate_dev, int max_cell_points, int32_t *info_dev, void *scratch_dev,
                       void *stream) {
  return ndt_update_impl(c, &sps_ctx::ndt_map, NDT_MAP_NOT_DYNAMIC, pts_dev, n_dev, cap, T_host, T_dev, gate_dev,
                         max_cell_points, info_dev, scratch_dev, stream);
}

int sps_ndt_map_info(sps_ctx *c, int64_t *out_host) {
  return ndt_info_impl(c, &sps_ctx::ndt_map, NDT_MAP_NOT_DYNAMIC, 0, out_host);
}

int64_t sps_ndt_map_carve_scratch(int64_t cap) { return sps_ndt_pyramid_carve_scratch(cap, 1); }

int sps_ndt_map_carve(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                      const double *T_dev, const int32_t *gate_dev, double end_margin, double through_sigma, int min_pass,
                      int miss_frames, int max_steps, int32_t *info_dev, void *scratch_dev, void *stream) {
  (void)scratch_dev;   // sps_ndt_map_carve_scratch is 0
  return ndt_carve_impl(c, &sps_ctx::ndt_map, NDT_MAP_NOT_DYNAMIC, pts_dev, n_dev, cap, T_host, T_dev, gate_dev, &end_margin,
                        through_sigma, min_pass, miss_frames, max_steps, info_dev, stream);
}

int sps_ndt_map_carve_cells(sps_ctx *c, int32_t *pass_out_dev, int32_t *hit_out_dev, int32_t *miss_out_dev) {
  return ndt_carve_cells_impl(c, &sps_ctx::ndt_map, NDT_MAP_NOT_DYNAMIC, 0, pass_out_dev, hit_out_dev, miss_out_dev);
}

// ---- the pyramid -----------------------------------------------------------------------------------------------------------
int sps_ndt_pyramid_build_dynamic(sps_ctx *c, int n_levels, const uint64_t *const *cell_keys_dev,
                                  const int32_t *const *cell_start_dev, const int32_t *const *cell_pts_dev, const int64_t *n_cells,
                                  const double *resolution, const double *map_xyz_dev, int64_t n_map, int min_points,
                                  double eig_ratio, double outlier_ratio, const int64_t *cell_capacity, void *stream) {
  if (!cell_capacity) return fail(SPS_ERR_INVALID, "bad arguments");
  return ndt_build_impl(c, &sps_ctx::ndt_pyr, n_levels, cell_keys_dev, cell_start_dev, cell_pts_dev, n_cells, resolution,
                        map_xyz_dev, n_map, min_points, eig_ratio, &outlier_ratio, cell_capacity, stream);
}

int64_t sps_ndt_pyramid_update_scratch(int64_t cap, int n_levels) {
  if (!ndt_online_cap_ok(cap) || n_levels < 1 || n_levels > NDT_PYR_MAX) return -1;
  return (int64_t)ndt_pyr_upd_layout(cap, n_levels, nullptr, nullptr, nullptr);
}

int sps_ndt_pyramid_update(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                           const double *T_dev, const int32_t *gate_dev, int max_cell_points, int32_t *info_dev,
                           void *scratch_dev, void *stream) {
  return ndt_update_impl(c, &sps_ctx::ndt_pyr, NDT_PYR_NOT_DYNAMIC, pts_dev, n_dev, cap, T_host, T_dev, gate_dev,
                         max_cell_points, info_dev, scratch_dev, stream);
}

int64_t sps_ndt_pyramid_carve_scratch(int64_t cap, int n_levels) {
  if (!ndt_online_cap_ok(cap) || n_levels < 1 || n_levels > NDT_PYR_MAX) return -1;
  return 0;
}

int sps_ndt_pyramid_carve(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                          const double *T_dev, const int32_t *gate_dev, const double *end_margin, double through_sigma,
                          int min_pass, int miss_frames, int max_steps, int32_t *info_dev, void *scratch_dev, void *stream) {
  (void)scratch_dev;   // sps_ndt_pyramid_carve_scratch is 0
  return ndt_carve_impl(c, &sps_ctx::ndt_pyr, NDT_PYR_NOT_DYNAMIC, pts_dev, n_dev, cap, T_host, T_dev, gate_dev, end_margin,
                        through_sigma, min_pass, miss_frames, max_steps, info_dev, stream);
}

int sps_ndt_pyramid_info(sps_ctx *c, int level, int64_t *out_host) {
  return ndt_info_impl(c, &sps_ctx::ndt_pyr, NDT_PYR_NOT_DYNAMIC, level, out_host);
}

int sps_ndt_pyramid_carve_cells(sps_ctx *c, int level, int32_t *pass_out_dev, int32_t *hit_out_dev, int32_t *miss_out_dev) {
  return ndt_carve_cells_impl(c, &sps_ctx::ndt_pyr, NDT_PYR_NOT_DYNAMIC, level, pass_out_dev, hit_out_dev, miss_out_dev);
}
