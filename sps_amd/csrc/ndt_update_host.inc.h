// ndt_update_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_search_host.inc.h): the
// online NDT map (ABI: the "NDT localiser, online map" section of include/sps_hip.h; kernels: ndt_update_kernels.inc.h).
// sps_ndt_map_build_dynamic is sps_ndt_map_build with a cell capacity (ndt_map_build_impl, ndt_host.inc.h): it allocates and
// synchronises; sps_ndt_map_update does neither.

namespace {
inline size_t ndt_upd_align(size_t v) { return (v + 255) & ~(size_t)255; }

// the caller's scratch cut into its arrays (base == nullptr: only the size is wanted)
inline size_t ndt_upd_layout(int64_t cap, char *base, NdtUpdScratch *s) {
  const size_t n = (size_t)(cap < 1 ? 1 : cap), hs = (size_t)ndt_hash_slots(cap);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char *p = base ? base + at : nullptr;
    at += ndt_upd_align(bytes);
    return p;
  };
  char *q = take(n * 3 * 8), *bstat = take(n * 10 * 8), *hkeys = take(hs * 8), *cell_of = take(n * 4), *slot_of = take(n * 4),
       *list = take(n * 4), *tcell = take(n * 4), *hfirst = take(hs * 4), *hrank = take(hs * 4), *nt = take(4);
  if (s) {
    s->q = (double *)q, s->bstat = (double *)bstat, s->cell_of = (int *)cell_of, s->slot_of = (int *)slot_of;
    s->list = (int *)list, s->tcell = (int *)tcell, s->n_touched = (int *)nt;
    s->h.keys = (uint64_t *)hkeys, s->h.first = (int *)hfirst, s->h.rank = (int *)hrank, s->h.mask = (uint32_t)(hs - 1);
  }
  return at;
}
}  // namespace

int sps_ndt_map_build_dynamic(sps_ctx *c, const uint64_t *cell_keys_dev, const int32_t *cell_start_dev,
                              const int32_t *cell_pts_dev, const double *map_xyz_dev, int64_t n_cells, int64_t n_map,
                              double resolution, int min_points, double eig_ratio, int64_t cell_capacity, void *stream) {
  return ndt_map_build_impl(c, cell_keys_dev, cell_start_dev, cell_pts_dev, map_xyz_dev, n_cells, n_map, resolution, min_points,
                            eig_ratio, true, cell_capacity, stream);
}

int64_t sps_ndt_map_update_scratch(int64_t cap) {
  if (cap < 0 || cap > SPS_NDT_UPDATE_MAX_POINTS) return -1;
  return (int64_t)ndt_upd_layout(cap, nullptr, nullptr);
}

int sps_ndt_map_update(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                       const double *T_dev, const int32_t *gate_dev, int max_cell_points, int32_t *info_dev, void *scratch_dev,
                       void *stream) {
  if (!c || !n_dev || !info_dev || !scratch_dev || cap < 0 || (cap > 0 && !pts_dev) || (!T_host && !T_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (!c->ndt.h.keys || c->ndt_dyn.capacity <= 0)
    return fail(SPS_ERR_INVALID, "the map of this context is not dynamic (sps_ndt_map_build_dynamic)");
  if (cap > SPS_NDT_UPDATE_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_NDT_UPDATE_MAX_POINTS);
  if (max_cell_points < 0) return fail(SPS_ERR_INVALID, "max_cell_points must be >= 0");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  LocPose Th{};
  if (T_host)
    for (int i = 0; i < 16; ++i) Th.m[i] = T_host[i];
  NdtUpdScratch s{};
  ndt_upd_layout(cap, (char *)scratch_dev, &s);
  const size_t hs = (size_t)s.h.mask + 1;
  const NdtDyn &d = c->ndt_dyn;
  const int nbp = (int)((cap + 255) / 256 > 0 ? (cap + 255) / 256 : 1);
  const int nbs = (int)std::min<int64_t>(std::max<int64_t>(cap / 4, 1), 2048);
  // the update's own hash starts empty whatever the gate says: it is scratch
  HIP_TRY(hipMemsetAsync(s.h.keys, 0xFF, hs * 8, st));
  HIP_TRY(hipMemsetAsync(s.h.first, 0x7F, hs * 4, st));
  hipLaunchKernelGGL(k_ndt_upd_lookup, dim3(nbp), dim3(256), 0, st, pts_dev, n_dev, (int)cap, Th, T_dev, gate_dev, c->ndt, s);
  hipLaunchKernelGGL(k_ndt_upd_found, dim3(1), dim3(NDT_UPD_BLOCK), 0, st, n_dev, (int)cap, gate_dev, d, s, info_dev);
  hipLaunchKernelGGL(k_ndt_upd_resolve, dim3(nbp), dim3(256), 0, st, n_dev, (int)cap, gate_dev, c->ndt, d, s);
  hipLaunchKernelGGL(k_ndt_upd_offsets, dim3(1), dim3(NDT_UPD_BLOCK), 0, st, n_dev, (int)cap, gate_dev, d, s, info_dev);
  hipLaunchKernelGGL(k_ndt_upd_fill, dim3(nbp), dim3(256), 0, st, n_dev, (int)cap, gate_dev, d, s);
  hipLaunchKernelGGL(k_ndt_upd_stats, dim3(nbs), dim3(64), 0, st, n_dev, (int)cap, gate_dev, d, s);
  hipLaunchKernelGGL(k_ndt_upd_merge, dim3(nbp), dim3(256), 0, st, n_dev, (int)cap, gate_dev, max_cell_points, d, s);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int sps_ndt_map_info(sps_ctx *c, int64_t *out_host) {
  if (!c || !out_host) return fail(SPS_ERR_INVALID, "bad arguments");
  if (!c->ndt.h.keys || c->ndt_dyn.capacity <= 0)
    return fail(SPS_ERR_INVALID, "the map of this context is not dynamic (sps_ndt_map_build_dynamic)");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  int32_t st[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpy(st, c->ndt_dyn.state, sizeof(st), hipMemcpyDeviceToHost));
  out_host[0] = st[0], out_host[1] = c->ndt_dyn.capacity, out_host[2] = st[1], out_host[3] = 0;
  return SPS_OK;
}
