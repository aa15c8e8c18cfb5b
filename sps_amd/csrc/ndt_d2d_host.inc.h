// ndt_d2d_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_pyramid_host.inc.h): the entry
// points of distribution-to-distribution NDT (ABI: the "NDT localiser, distribution to distribution" sections of
// include/sps_hip.h: the single call, several poses, the pyramid; kernels: ndt_d2d_kernels.inc.h).
// No call allocates or synchronises: the scratch is the caller's.  The single source build and the pyramid of sources share
// ndt_src_layout and the kernels' bodies and keep their own launches; the batch, the score and the pyramid alignment are the
// implementations of ndt_batch_host.inc.h, ndt_search_host.inc.h and ndt_pyramid_host.inc.h with the kernels of NdtCells,
// their scratch layouts those of the point versions with the source capacity in place of the point capacity.

namespace {
// The source build's scratch: the update's own arrays and, beside them, the empty map that the update's bodies found the
// scan's cells in.  Arrays that start from the same byte lie together, so one memset serves each value:
//   0xFF  the update's hash keys, the map's hash keys, the map's hash ranks
//   0x7F  the update's hash `first`, the cells' `lead`
//   0     the cells' `bcnt`, the map's state words
// It is array-major: every array holds the n_levels levels back to back, so the three memsets serve any number of levels.
// s, m and d are level 0's views and w what turns them into level l's (ndt_pyr_upd_slice, ndt_pyr_src_map,
// ndt_pyr_src_dyn); info: int[n_levels][4].  One level is the single build's layout.
struct NdtSrcLayout {
  NdtUpdScratch s;
  NdtMap m;
  NdtDyn d;
  NdtPyrUpdStride w;
  int *info;
  char *ff, *sf, *zero;
  size_t ff_bytes, sf_bytes, zero_bytes;
};
inline size_t ndt_src_layout(int64_t cap, int n_levels, char *base, NdtSrcLayout *L) {
  const size_t n = (size_t)(cap < 1 ? 1 : cap), hs = (size_t)ndt_hash_slots(cap), l = (size_t)n_levels;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char *p = base ? base + at : nullptr;
    at += ndt_upd_align(bytes);
    return p;
  };
  char *shkeys = take(l * hs * 8), *mhkeys = take(l * hs * 8), *mhrank = take(l * hs * 4);
  const size_t ff_end = at;
  char *shfirst = take(l * hs * 4), *lead = take(l * n * 4);
  const size_t sf_end = at;
  char *bcnt = take(l * n * 4), *state = take(l * 16);
  const size_t zero_end = at;
  char *q = take(n * 3 * 8), *bstat = take(l * n * 10 * 8), *cell_of = take(l * n * 4), *slot_of = take(l * n * 4),
       *list = take(l * n * 4), *tcell = take(l * n * 4), *shrank = take(l * hs * 4), *nt = take(l * 4), *cstart = take(l * n * 4),
       *keys = take(l * n * 8), *info = take(l * 16);
  if (L) {
    NdtUpdScratch &s = L->s;
    s.q = (double *)q, s.bstat = (double *)bstat, s.cell_of = (int *)cell_of, s.slot_of = (int *)slot_of;
    s.list = (int *)list, s.tcell = (int *)tcell, s.n_touched = (int *)nt;
    s.h.keys = (uint64_t *)shkeys, s.h.first = (int *)shfirst, s.h.rank = (int *)shrank, s.h.mask = (uint32_t)(hs - 1);
    L->m = NdtMap{};
    L->m.h.keys = (uint64_t *)mhkeys, L->m.h.first = nullptr, L->m.h.rank = (int *)mhrank, L->m.h.mask = (uint32_t)(hs - 1);
    L->m.n_cells = (int)n;                                 // rec, count and keys are not read by the bodies used; a
                                                           // level's resolution is set on the device
    L->d = NdtDyn{};
    L->d.capacity = (int)n;                                // room for every point's own cell: nothing is ever dropped
    L->d.keys = (uint64_t *)keys, L->d.bcnt = (int *)bcnt, L->d.lead = (int *)lead, L->d.cstart = (int *)cstart;
    L->d.state = (int *)state;
    L->w.n = (int)n, L->w.hs = (int)hs;
    L->info = (int *)info;
    L->ff = shkeys, L->ff_bytes = ff_end;
    L->sf = shfirst, L->sf_bytes = sf_end - ff_end;
    L->zero = bcnt, L->zero_bytes = zero_end - sf_end;
  }
  return at;
}
}  // namespace

int64_t sps_ndt_source_scratch(int64_t cap) {
  if (cap < 0 || cap > SPS_NDT_UPDATE_MAX_POINTS) return -1;
  return (int64_t)ndt_src_layout(cap, 1, nullptr, nullptr);
}

int64_t sps_ndt_pyramid_source_scratch(int64_t cap, int n_levels) {
  if (cap < 0 || cap > SPS_NDT_UPDATE_MAX_POINTS || n_levels < 1 || n_levels > NDT_PYR_MAX) return -1;
  return (int64_t)ndt_src_layout(cap, n_levels, nullptr, nullptr);
}

int sps_ndt_source_build(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, double source_resolution,
                         int min_points, double eig_ratio, double *src_dev, int32_t *src_count_dev, int32_t *n_src_dev,
                         void *scratch_dev, void *stream) {
  if (!c || !n_dev || !n_src_dev || !scratch_dev || cap < 0 || (cap > 0 && (!pts_dev || !src_dev)))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (cap > SPS_NDT_UPDATE_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_NDT_UPDATE_MAX_POINTS);
  if (!(source_resolution > 0.0) || std::isinf(source_resolution))
    return fail(SPS_ERR_INVALID, "source_resolution must be finite and > 0");
  if (!(eig_ratio > 0.0) || !(eig_ratio <= 1.0)) return fail(SPS_ERR_INVALID, "eig_ratio must be in (0, 1]");
  if (min_points < 0) return fail(SPS_ERR_INVALID, "min_points must be >= 0");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  NdtSrcLayout L{};
  ndt_src_layout(cap, 1, (char *)scratch_dev, &L);
  L.m.resolution = source_resolution;
  LocPose I{};
  I.m[0] = I.m[5] = I.m[10] = I.m[15] = 1.0;
  const int nbp = (int)((cap + 255) / 256 > 0 ? (cap + 255) / 256 : 1);
  const int nbs = (int)std::min<int64_t>(std::max<int64_t>(cap / 4, 1), 2048);
  HIP_TRY(hipMemsetAsync(L.ff, 0xFF, L.ff_bytes, st));
  HIP_TRY(hipMemsetAsync(L.sf, 0x7F, L.sf_bytes, st));
  HIP_TRY(hipMemsetAsync(L.zero, 0, L.zero_bytes, st));
  HIP_TRY(hipMemsetAsync(n_src_dev, 0, 2 * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_ndt_src_lookup, dim3(nbp), dim3(256), 0, st, pts_dev, n_dev, (int)cap, I, L.m, L.s);
  hipLaunchKernelGGL(k_ndt_src_found, dim3(1), dim3(NDT_UPD_BLOCK), 0, st, n_dev, (int)cap, L.d, L.s, L.info);
  hipLaunchKernelGGL(k_ndt_src_resolve, dim3(nbp), dim3(256), 0, st, n_dev, (int)cap, L.m, L.d, L.s);
  hipLaunchKernelGGL(k_ndt_src_offsets, dim3(1), dim3(NDT_UPD_BLOCK), 0, st, n_dev, (int)cap, L.d, L.s, L.info);
  hipLaunchKernelGGL(k_ndt_src_fill, dim3(nbp), dim3(256), 0, st, n_dev, (int)cap, L.d, L.s);
  hipLaunchKernelGGL(k_ndt_src_stats, dim3(nbs), dim3(64), 0, st, n_dev, (int)cap, L.d, L.s);
  hipLaunchKernelGGL(k_ndt_src_records, dim3(nbp), dim3(256), 0, st, n_dev, (int)cap, min_points, eig_ratio, L.s, src_dev,
                     src_count_dev, n_src_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
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
  ndt_src_layout(cap, n_levels, (char *)scratch_dev, &Y);
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

// ---- the alignments and the score: the point versions' implementations with the kernels of NdtCells ---------------------
int64_t sps_ndt_align_d2d_scratch(int64_t cap_src) { return sps_loc_align_scratch(cap_src); }   // the partial rows of k_loc_solve

int sps_ndt_align_d2d(sps_ctx *c, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src, const double *T_init_host,
                      int iters, int neighbours, int min_corr, double outlier_ratio, double tol_t, double tol_r,
                      double *T_out_dev, int32_t *status_dev, double *trace_dev, double *normal_dev, void *scratch_dev,
                      void *stream) {
  if (!c || !n_src_dev || !T_init_host || !T_out_dev || !status_dev || !scratch_dev || cap_src < 0 || iters < 0 ||
      (cap_src > 0 && !src_dev) || (iters > 0 && !trace_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  NdtGauss gs;
  if (int e = ndt_check_scan_args(c, neighbours, cap_src, outlier_ratio, gs, true, iters, tol_t, tol_r)) return e;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  LocPose T0;
  for (int i = 0; i < 16; ++i) T0.m[i] = T_init_host[i];
  const int nb = (int)loc_align_blocks(cap_src);
  double *partial = (double *)scratch_dev;
  int *done = (int *)(partial + (size_t)nb * LOC_TERMS);
  if (iters > 0) HIP_TRY(hipMemsetAsync(trace_dev, 0, (size_t)iters * 4 * sizeof(double), st));
  if (iters > 0 && normal_dev) HIP_TRY(hipMemsetAsync(normal_dev, 0, (size_t)iters * 28 * sizeof(double), st));
  hipLaunchKernelGGL(k_loc_init, dim3(1), dim3(64), 0, st, T0, T_out_dev, status_dev, done);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(k_ndt_d2d_assoc, dim3(nb), dim3(256), 0, st, src_dev, n_src_dev, (int)cap_src, c->ndt_map.lv[0].m, gs, neighbours,
                       (const double *)T_out_dev, (const int *)done, partial);
    hipLaunchKernelGGL(k_loc_solve, dim3(1), dim3(256), 0, st, (const double *)partial, n_src_dev, (int)cap_src, it, min_corr,
                       tol_t, tol_r, T0, T_out_dev, status_dev, done, trace_dev, normal_dev);
  }
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int64_t sps_ndt_align_d2d_batch_scratch(int64_t cap_src, int n_hyp) { return sps_ndt_align_batch_scratch(cap_src, n_hyp); }

int sps_ndt_align_d2d_batch(sps_ctx *c, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src, const double *T_init_dev,
                            int n_hyp, int iters, int neighbours, int min_corr, double outlier_ratio, double tol_t, double tol_r,
                            double *T_out_dev, int32_t *status_dev, double *trace_dev, double *normal_dev, double *final_dev,
                            int32_t *best_dev, double *T_best_dev, void *scratch_dev, void *stream) {
  return ndt_align_batch_impl(k_ndt_assoc_batch<NdtCells>, c, src_dev, n_src_dev, cap_src, T_init_dev, n_hyp, iters, neighbours,
                              min_corr, outlier_ratio, tol_t, tol_r, T_out_dev, status_dev, trace_dev, normal_dev, final_dev,
                              best_dev, T_best_dev, scratch_dev, stream);
}

int64_t sps_ndt_score_d2d_scratch(int64_t cap_src, int64_t n_pose) { return sps_ndt_score_scratch(cap_src, n_pose); }

int sps_ndt_score_poses_d2d(sps_ctx *c, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src, const double *T_dev,
                            int64_t n_pose, int neighbours, double outlier_ratio, double *score_dev, void *scratch_dev,
                            void *stream) {
  return ndt_score_poses_impl(k_ndt_score<NdtCells>, c, src_dev, n_src_dev, cap_src, T_dev, n_pose, neighbours, outlier_ratio,
                              score_dev, scratch_dev, stream);
}

// the partial rows of launch B (one per 32 sources), then the state words: sps_ndt_pyramid_align_scratch's layout
int64_t sps_ndt_pyramid_align_d2d_scratch(int64_t cap_src) { return sps_ndt_pyramid_align_scratch(cap_src); }

int sps_ndt_pyramid_align_d2d(sps_ctx *c, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src,
                              const double *T_init_host, int iters, const int32_t *level_iters, int neighbours, int min_corr,
                              double tol_t, double tol_r, double *T_out_dev, int32_t *status_dev, double *trace_dev,
                              double *normal_dev, int32_t *level_dev, void *scratch_dev, void *stream) {
  return ndt_pyramid_align_impl(k_ndt_pyr_assoc<NdtCells>, k_ndt_pyr_solve<NdtCells>, c, src_dev, n_src_dev, cap_src, T_init_host,
                                iters, level_iters, neighbours, min_corr, tol_t, tol_r, T_out_dev, status_dev, trace_dev,
                                normal_dev, level_dev, scratch_dev, stream);
}
