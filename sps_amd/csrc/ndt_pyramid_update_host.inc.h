// ndt_pyramid_update_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_pyramid_host.inc.h):
// the online NDT pyramid (ABI: the "NDT localiser, online pyramid" section of include/sps_hip.h; kernels:
// ndt_pyramid_update_kernels.inc.h).  sps_ndt_pyramid_build_dynamic is sps_ndt_pyramid_build with a cell
// capacity per level (ndt_pyramid_build_impl, ndt_pyramid_host.inc.h): it allocates and synchronises.
// sps_ndt_pyramid_update and sps_ndt_pyramid_carve do neither, and what they issue can be read off below: seven launches
// and two memsets, and three launches, whatever the number of levels and the data.

namespace {
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

// the context has a dynamic pyramid, or the error text is set
inline int ndt_pyr_check_dynamic(const sps_ctx *c) {
  if (c->ndt_pyr.n_levels < 1 || !c->ndt_pyr.dynamic || !c->ndt_pyr.dyn_dev)
    return fail(SPS_ERR_INVALID, "the pyramid of this context is not dynamic (sps_ndt_pyramid_build_dynamic)");
  return SPS_OK;
}
}  // namespace

int sps_ndt_pyramid_build_dynamic(sps_ctx *c, int n_levels, const uint64_t *const *cell_keys_dev,
                                  const int32_t *const *cell_start_dev, const int32_t *const *cell_pts_dev, const int64_t *n_cells,
                                  const double *resolution, const double *map_xyz_dev, int64_t n_map, int min_points,
                                  double eig_ratio, double outlier_ratio, const int64_t *cell_capacity, void *stream) {
  if (!cell_capacity) return fail(SPS_ERR_INVALID, "bad arguments");
  return ndt_pyramid_build_impl(c, n_levels, cell_keys_dev, cell_start_dev, cell_pts_dev, n_cells, resolution, map_xyz_dev, n_map,
                                min_points, eig_ratio, outlier_ratio, cell_capacity, stream);
}

int64_t sps_ndt_pyramid_update_scratch(int64_t cap, int n_levels) {
  if (cap < 0 || cap > SPS_NDT_UPDATE_MAX_POINTS || n_levels < 1 || n_levels > NDT_PYR_MAX) return -1;
  return (int64_t)ndt_pyr_upd_layout(cap, n_levels, nullptr, nullptr, nullptr);
}

int sps_ndt_pyramid_update(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                           const double *T_dev, const int32_t *gate_dev, int max_cell_points, int32_t *info_dev,
                           void *scratch_dev, void *stream) {
  if (!c || !n_dev || !info_dev || !scratch_dev || cap < 0 || (cap > 0 && !pts_dev) || (!T_host && !T_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (int e = ndt_pyr_check_dynamic(c)) return e;
  if (cap > SPS_NDT_UPDATE_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_NDT_UPDATE_MAX_POINTS);
  if (max_cell_points < 0) return fail(SPS_ERR_INVALID, "max_cell_points must be >= 0");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  LocPose Th{};
  if (T_host)
    for (int i = 0; i < 16; ++i) Th.m[i] = T_host[i];
  const unsigned L = (unsigned)c->ndt_pyr.n_levels;
  NdtUpdScratch s{};
  NdtPyrUpdStride w{};
  ndt_pyr_upd_layout(cap, (int)L, (char *)scratch_dev, &s, &w);
  const NdtPyrLevel *lv = c->ndt_pyr.dev;
  const NdtDyn *dy = c->ndt_pyr.dyn_dev;
  const unsigned nbp = (unsigned)((cap + 255) / 256 > 0 ? (cap + 255) / 256 : 1);
  const unsigned nbs = (unsigned)std::min<int64_t>(std::max<int64_t>(cap / 4, 1), 2048);
  // the levels' update hashes start empty whatever the gate says: they are scratch.  Two memsets cover all levels.
  HIP_TRY(hipMemsetAsync(s.h.keys, 0xFF, (size_t)L * (size_t)w.hs * 8, st));
  HIP_TRY(hipMemsetAsync(s.h.first, 0x7F, (size_t)L * (size_t)w.hs * 4, st));
  hipLaunchKernelGGL(k_ndt_pyr_upd_lookup, dim3(nbp, L), dim3(256), 0, st, pts_dev, n_dev, (int)cap, Th, T_dev, gate_dev, lv, s, w);
  hipLaunchKernelGGL(k_ndt_pyr_upd_found, dim3(1, L), dim3(NDT_UPD_BLOCK), 0, st, n_dev, (int)cap, gate_dev, dy, s, w, info_dev);
  hipLaunchKernelGGL(k_ndt_pyr_upd_resolve, dim3(nbp, L), dim3(256), 0, st, n_dev, (int)cap, gate_dev, lv, dy, s, w);
  hipLaunchKernelGGL(k_ndt_pyr_upd_offsets, dim3(1, L), dim3(NDT_UPD_BLOCK), 0, st, n_dev, (int)cap, gate_dev, dy, s, w, info_dev);
  hipLaunchKernelGGL(k_ndt_pyr_upd_fill, dim3(nbp, L), dim3(256), 0, st, n_dev, (int)cap, gate_dev, dy, s, w);
  hipLaunchKernelGGL(k_ndt_pyr_upd_stats, dim3(nbs, L), dim3(64), 0, st, n_dev, (int)cap, gate_dev, dy, s, w);
  hipLaunchKernelGGL(k_ndt_pyr_upd_merge, dim3(nbp, L), dim3(256), 0, st, n_dev, (int)cap, gate_dev, max_cell_points, dy, s, w);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int64_t sps_ndt_pyramid_carve_scratch(int64_t cap, int n_levels) {
  if (cap < 0 || cap > SPS_NDT_UPDATE_MAX_POINTS || n_levels < 1 || n_levels > NDT_PYR_MAX) return -1;
  return 0;
}

int sps_ndt_pyramid_carve(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                          const double *T_dev, const int32_t *gate_dev, const double *end_margin, double through_sigma,
                          int min_pass, int miss_frames, int max_steps, int32_t *info_dev, void *scratch_dev, void *stream) {
  (void)scratch_dev;   // sps_ndt_pyramid_carve_scratch is 0
  if (!c || !n_dev || !info_dev || !end_margin || cap < 0 || (cap > 0 && !pts_dev) || (!T_host && !T_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (int e = ndt_pyr_check_dynamic(c)) return e;
  if (cap > SPS_NDT_UPDATE_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_NDT_UPDATE_MAX_POINTS);
  const int L = c->ndt_pyr.n_levels;
  NdtPyrMargins em{};
  int cmax = 1;
  for (int l = 0; l < L; ++l) {
    if (!(end_margin[l] >= 0.0) || std::isinf(end_margin[l])) return fail(SPS_ERR_INVALID, "end_margin must be finite and >= 0");
    em.v[l] = end_margin[l];
    cmax = std::max(cmax, c->ndt_pyr.dyn[l].capacity);
  }
  if (!(through_sigma > 0.0) || std::isinf(through_sigma)) return fail(SPS_ERR_INVALID, "through_sigma must be finite and > 0");
  if (min_pass < 1 || miss_frames < 1) return fail(SPS_ERR_INVALID, "min_pass and miss_frames must be >= 1");
  if (max_steps < 1 || max_steps > 4096) return fail(SPS_ERR_INVALID, "max_steps must be in [1, 4096]");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  LocPose Th{};
  if (T_host)
    for (int i = 0; i < 16; ++i) Th.m[i] = T_host[i];
  const NdtPyrLevel *lv = c->ndt_pyr.dev;
  const NdtDyn *dy = c->ndt_pyr.dyn_dev;
  const NdtCarveParams p{0.0, through_sigma * through_sigma, min_pass, miss_frames, max_steps};   // end_margin: per level, em
  const unsigned nbp = (unsigned)((cap + 255) / 256 > 0 ? (cap + 255) / 256 : 1);
  const unsigned nbc = (unsigned)((cmax + 255) / 256);   // the largest level's; a smaller level's surplus threads return
  hipLaunchKernelGGL(k_ndt_pyr_carve_begin, dim3(nbc, (unsigned)L), dim3(256), 0, st, gate_dev, dy, info_dev);
  hipLaunchKernelGGL(k_ndt_pyr_carve_rays, dim3(nbp, (unsigned)L), dim3(256), 0, st, pts_dev, n_dev, (int)cap, Th, T_dev, gate_dev, lv,
                     dy, p, em, info_dev);
  hipLaunchKernelGGL(k_ndt_pyr_carve_decide, dim3(nbc, (unsigned)L), dim3(256), 0, st, gate_dev, dy, p, info_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int sps_ndt_pyramid_info(sps_ctx *c, int level, int64_t *out_host) {
  if (!c || !out_host) return fail(SPS_ERR_INVALID, "bad arguments");
  if (int e = ndt_pyr_check_dynamic(c)) return e;
  if (level < 0 || level >= c->ndt_pyr.n_levels) return fail(SPS_ERR_INVALID, "level must be in [0, %d)", c->ndt_pyr.n_levels);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  const NdtDyn &d = c->ndt_pyr.dyn[level];
  int32_t st[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpy(st, d.state, sizeof(st), hipMemcpyDeviceToHost));
  out_host[0] = st[0], out_host[1] = d.capacity, out_host[2] = st[1], out_host[3] = 0;
  return SPS_OK;
}

int sps_ndt_pyramid_carve_cells(sps_ctx *c, int level, int32_t *pass_out_dev, int32_t *hit_out_dev, int32_t *miss_out_dev) {
  if (!c) return fail(SPS_ERR_INVALID, "ctx is null");
  if (int e = ndt_pyr_check_dynamic(c)) return e;
  if (level < 0 || level >= c->ndt_pyr.n_levels) return fail(SPS_ERR_INVALID, "level must be in [0, %d)", c->ndt_pyr.n_levels);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  const NdtDyn &d = c->ndt_pyr.dyn[level];
  const size_t bytes = (size_t)d.capacity * sizeof(int32_t);
  if (pass_out_dev) HIP_TRY(hipMemcpy(pass_out_dev, d.pass, bytes, hipMemcpyDeviceToDevice));
  if (hit_out_dev) HIP_TRY(hipMemcpy(hit_out_dev, d.hit, bytes, hipMemcpyDeviceToDevice));
  if (miss_out_dev) HIP_TRY(hipMemcpy(miss_out_dev, d.miss, bytes, hipMemcpyDeviceToDevice));
  HIP_TRY(hipDeviceSynchronize());
  return SPS_OK;
}
