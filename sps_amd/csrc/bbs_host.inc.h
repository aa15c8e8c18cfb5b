// bbs_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_search_host.inc.h): the entry
// points of the global search (ABI: the "NDT localiser, global search" section of include/sps_hip.h; kernels:
// bbs_kernels.inc.h).  sps_bbs_map_build allocates and synchronises, like sps_ndt_map_build; sps_bbs_search does neither:
// its scratch is the caller's.

namespace {
inline int64_t bbs_align(int64_t v) { return (v + 255) & ~(int64_t)255; }
// the arrays cut from the caller's scratch, in bytes from its start
struct BbsScratch {
  int64_t offs, hist, ctl, score, cand_a, cand_b, sums_a, sums_t, total;
};
inline BbsScratch bbs_scratch_layout(int64_t cap, int64_t n_yaw, int64_t frontier) {
  BbsScratch s{};
  const int64_t slots = 4 * frontier, blocks = (slots + SCAN_BLOCK - 1) / SCAN_BLOCK;
  int64_t at = 0;
  auto cut = [&](int64_t bytes) {
    const int64_t here = at;
    at += bbs_align(bytes);
    return here;
  };
  s.offs = cut(n_yaw * std::max<int64_t>(cap, 1) * 4);
  s.hist = cut((int64_t)BBS_HIST * 4);
  s.ctl = cut(BBS_C_WORDS * 4);
  s.score = cut(slots * 4);
  s.cand_a = cut(slots * 4);
  s.cand_b = cut(slots * 4);
  s.sums_a = cut(blocks * 4);
  s.sums_t = cut(blocks * 4);
  s.total = at;
  return s;
}
inline bool bbs_sizes_ok(int64_t cap, int64_t n_yaw, int64_t frontier) {
  return cap >= 0 && cap <= BBS_MAX_POINTS && n_yaw >= 1 && n_yaw <= SPS_BBS_MAX_YAWS && frontier >= 1 &&
         frontier <= SPS_BBS_MAX_FRONTIER;
}
}  // namespace

int sps_bbs_map_build(sps_ctx *c, const uint8_t *g0_dev, int64_t W, int64_t H, int levels, void *stream) {
  if (!c || !g0_dev) return fail(SPS_ERR_INVALID, "bad arguments");
  if (levels < 0 || levels >= BBS_MAX_LEVELS) return fail(SPS_ERR_INVALID, "levels must be in [0, %d]", BBS_MAX_LEVELS - 1);
  const int64_t pad = (1ll << levels) - 1;
  if (W < 1 || H < 1 || W + pad > BBS_MAX_STORE || H + pad > BBS_MAX_STORE)
    return fail(SPS_ERR_INVALID, "W and H must be >= 1 and, with 2^levels - 1 added, <= %d", BBS_MAX_STORE);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipDeviceSynchronize());                         // a search in flight may still read the old pyramid
  if (c->bbs_alloc) (void)hipFree(c->bbs_alloc);
  c->bbs_alloc = nullptr, c->bbs = BbsGrid{};
  BbsGrid b{};
  b.W = (int)W, b.H = (int)H, b.pad = (int)pad, b.L = levels, b.Ws = (int)(W + pad), b.Hs = (int)(H + pad);
  const size_t level_bytes = (size_t)b.Ws * b.Hs;
  unsigned char *g = nullptr;
  if (hipMalloc((void **)&g, level_bytes * (levels + 1)) != hipSuccess) return fail(SPS_ERR_NOMEM, "hipMalloc for the occupancy pyramid failed");
  c->bbs_alloc = g;
  b.g = g;
  const unsigned nb = (unsigned)((level_bytes + 255) / 256);
  hipLaunchKernelGGL(k_bbs_pad, dim3(nb), dim3(256), 0, st, (const unsigned char *)g0_dev, b, g);
  for (int l = 1; l <= levels; ++l)
    hipLaunchKernelGGL(k_bbs_pool, dim3(nb), dim3(256), 0, st, b, l, (const unsigned char *)(g + (l - 1) * level_bytes),
                       g + l * level_bytes);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  c->bbs = b;
  return SPS_OK;
}

int sps_bbs_map_level(sps_ctx *c, int level, uint8_t *out_dev) {
  if (!c || !out_dev) return fail(SPS_ERR_INVALID, "bad arguments");
  if (!c->bbs.g) return fail(SPS_ERR_INVALID, "sps_bbs_map_build has not been called");
  if (level < 0 || level > c->bbs.L) return fail(SPS_ERR_INVALID, "level must be in [0, %d]", c->bbs.L);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t level_bytes = (size_t)c->bbs.Ws * c->bbs.Hs;
  HIP_TRY(hipMemcpy(out_dev, c->bbs.g + level * level_bytes, level_bytes, hipMemcpyDeviceToDevice));
  HIP_TRY(hipDeviceSynchronize());
  return SPS_OK;
}

int64_t sps_bbs_search_scratch(int64_t cap, int64_t n_yaw, int64_t frontier) {
  if (!bbs_sizes_ok(cap, n_yaw, frontier)) return -1;
  return bbs_scratch_layout(cap, n_yaw, frontier).total;
}

int sps_bbs_search(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_up_host,
                   double resolution, int64_t i0, int64_t j0, double scan_z_lo, double scan_z_hi, const double *yaw_cs_dev,
                   int64_t n_yaw, int64_t frontier, int min_score, int k, int32_t *top_index_dev, int32_t *top_score_dev,
                   double *T_top_dev, int32_t *n_top_dev, int32_t *info_dev, int32_t *trace_dev, void *scratch_dev,
                   void *stream) {
  if (!c || !n_dev || !T_up_host || !yaw_cs_dev || !top_index_dev || !top_score_dev || !T_top_dev || !n_top_dev || !info_dev ||
      !scratch_dev || cap < 0 || (cap > 0 && !pts_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (!c->bbs.g) return fail(SPS_ERR_INVALID, "sps_bbs_map_build has not been called");
  if (!bbs_sizes_ok(cap, n_yaw, frontier))
    return fail(SPS_ERR_INVALID, "cap must be <= %d, n_yaw in [1, %d] and frontier in [1, %d]", BBS_MAX_POINTS, SPS_BBS_MAX_YAWS,
                SPS_BBS_MAX_FRONTIER);
  if (k < 1 || k > SPS_NDT_MAX_HYP) return fail(SPS_ERR_INVALID, "k must be in [1, %d]", SPS_NDT_MAX_HYP);
  if (min_score < 0) return fail(SPS_ERR_INVALID, "min_score must be >= 0");
  if (!(resolution > 0.0) || std::isinf(resolution)) return fail(SPS_ERR_INVALID, "resolution must be finite and > 0");
  if (std::isnan(scan_z_lo) || std::isnan(scan_z_hi)) return fail(SPS_ERR_INVALID, "the scan slice must not be NaN");
  if (i0 < -(1ll << 30) || i0 > (1ll << 30) || j0 < -(1ll << 30) || j0 > (1ll << 30)) return fail(SPS_ERR_INVALID, "i0 or j0 out of range");
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(T_up_host[i])) return fail(SPS_ERR_INVALID, "T_up must be finite");
  const BbsGrid b = c->bbs;
  if (n_yaw * (int64_t)b.H * b.W >= (1ll << 31)) return fail(SPS_ERR_INVALID, "n_yaw * H * W must fit int32");
  const int64_t ni = (b.W + (1 << b.L) - 1) >> b.L, nj = (b.H + (1 << b.L) - 1) >> b.L;
  const int64_t n_root = n_yaw * nj * ni;
  if (n_root > 4 * frontier)
    return fail(SPS_ERR_INVALID, "%lld candidates at level %d exceed 4 * frontier = %lld", (long long)n_root, b.L, (long long)(4 * frontier));
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const BbsScratch sl = bbs_scratch_layout(cap, n_yaw, frontier);
  char *base = (char *)scratch_dev;
  int *offs = (int *)(base + sl.offs), *hist = (int *)(base + sl.hist), *ctl = (int *)(base + sl.ctl);
  int *score = (int *)(base + sl.score), *sums_a = (int *)(base + sl.sums_a), *sums_t = (int *)(base + sl.sums_t);
  int *lists[2] = {(int *)(base + sl.cand_a), (int *)(base + sl.cand_b)};
  LocPose U;
  for (int i = 0; i < 16; ++i) U.m[i] = T_up_host[i];
  const int F = (int)frontier;
  HIP_TRY(hipMemsetAsync(hist, 0, (size_t)BBS_HIST * 4, st));
  HIP_TRY(hipMemsetAsync(info_dev, 0, (size_t)BBS_INFO * 4, st));
  hipLaunchKernelGGL(k_bbs_offsets, dim3((unsigned)((std::max<int64_t>(cap, 1) + 255) / 256), (unsigned)n_yaw), dim3(256), 0, st,
                     pts_dev, n_dev, (int)cap, U, scan_z_lo, scan_z_hi, resolution, yaw_cs_dev, offs, info_dev + 3, ctl);
  const unsigned score_blocks = (unsigned)((4 * frontier + BBS_NODES - 1) / BBS_NODES);
  const unsigned scan_blocks = (unsigned)((4 * frontier + SCAN_BLOCK - 1) / SCAN_BLOCK);
  const int *cand = nullptr;                               // level L: the candidates are all root nodes, in their order
  const int *slots = ctl + BBS_C_SLOTS;                    // read from level L - 1 on, written by the level above
  int which = 0;
  for (int l = b.L; l >= 0; --l) {
    int *next = lists[which], *slots_out = ctl + (which ? BBS_C_SLOTS_B : BBS_C_SLOTS);
    hipLaunchKernelGGL(k_bbs_score, dim3(score_blocks), dim3(256), 0, st, cand, (int)n_root, slots, b, l,
                       (const int *)offs, n_dev, (int)cap, score, hist);
    hipLaunchKernelGGL(k_bbs_threshold, dim3(1), dim3(BBS_THR_THREADS), 0, st, hist, (int)cap, F, min_score, l, ctl, info_dev);
    hipLaunchKernelGGL(k_bbs_count, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, st, cand, (int)n_root, slots, (const int *)ctl,
                       (const int *)score, sums_a, sums_t);
    hipLaunchKernelGGL(k_bbs_write, dim3(scan_blocks), dim3(SCAN_BLOCK), 0, st, cand, (int)n_root, slots, (const int *)ctl, slots_out, b,
                       l, (const int *)score, (const int *)sums_a, (const int *)sums_t, F, next, trace_dev);
    cand = next, slots = slots_out;
    which ^= 1;
  }
  hipLaunchKernelGGL(k_bbs_top, dim3(1), dim3(NDT_TOP_THREADS), 0, st, cand, F, slots, (const int *)ctl, b, U, resolution, (int)i0, (int)j0,
                     yaw_cs_dev, k, top_index_dev, top_score_dev, T_top_dev, n_top_dev, info_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
