// ndt_search_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_batch_host.inc.h): the NDT
// score of many poses and the choice of the best of them (ABI: the "NDT localiser, pose search" section of
// include/sps_hip.h; kernels: ndt_search_kernels.inc.h).  Like sps_ndt_align_batch the calls neither allocate nor
// synchronise.

namespace {
constexpr int64_t NDT_SCORE_SCRATCH_MAX = 64ll << 20;   // the partial rows of one chunk of poses stay below this ...
// ... unless one tile of poses alone needs more.  Poses of one chunk: a multiple of the tile, at most n_pose.
inline int64_t ndt_score_chunk(int64_t cap, int64_t n_pose) {
  const int64_t row = loc_align_blocks(cap) * 16;       // bytes of one pose's partial rows
  int64_t chunk = (NDT_SCORE_SCRATCH_MAX / row) / NDT_SCORE_TILE * NDT_SCORE_TILE;
  if (chunk < NDT_SCORE_TILE) chunk = NDT_SCORE_TILE;
  return std::min(chunk, n_pose);
}

// the score of many poses with the scorer `score` (k_ndt_score of NdtPoints: sps_ndt_score_poses; of NdtCells:
// sps_ndt_score_poses_d2d)
int ndt_score_poses_impl(NdtScoreKernel score, sps_ctx *c, const double *elems_dev, const int32_t *n_dev, int64_t cap,
                         const double *T_dev, int64_t n_pose, int neighbours, double outlier_ratio, double *score_dev,
                         void *scratch_dev, void *stream) {
  if (!c || !n_dev || !T_dev || !score_dev || !scratch_dev || cap < 0 || (cap > 0 && !elems_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (n_pose < 1 || n_pose > SPS_NDT_MAX_POSES) return fail(SPS_ERR_INVALID, "n_pose must be in [1, %d]", SPS_NDT_MAX_POSES);
  NdtGauss gs;
  if (int e = ndt_check_scan_args(c, neighbours, cap, outlier_ratio, gs, false)) return e;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)loc_align_blocks(cap);
  const int64_t chunk = ndt_score_chunk(cap, n_pose);
  double *partial = (double *)scratch_dev;
  for (int64_t p0 = 0; p0 < n_pose; p0 += chunk) {      // chunks follow one another on the stream and share the scratch
    const int np = (int)std::min(chunk, n_pose - p0);
    hipLaunchKernelGGL(score, dim3(nb, (np + NDT_SCORE_TILE - 1) / NDT_SCORE_TILE), dim3(256), 0, st, elems_dev, n_dev,
                       (int)cap, c->ndt_map.lv[0].m, gs, neighbours, T_dev + p0 * 16, np, partial);
    hipLaunchKernelGGL(k_ndt_score_reduce, dim3((np + NDT_REDUCE_POSES - 1) / NDT_REDUCE_POSES), dim3(256), 0, st,
                       (const double *)partial, nb, n_dev, (int)cap, np, score_dev + p0 * 2);
  }
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
}  // namespace

int64_t sps_ndt_score_scratch(int64_t cap, int64_t n_pose) {
  if (cap < 0 || cap > SPS_MAX_POINTS || n_pose < 1 || n_pose > SPS_NDT_MAX_POSES) return -1;
  return ndt_score_chunk(cap, n_pose) * loc_align_blocks(cap) * 16;
}

int sps_ndt_score_poses(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_dev, int64_t n_pose,
                        int neighbours, double outlier_ratio, double *score_dev, void *scratch_dev, void *stream) {
  return ndt_score_poses_impl(k_ndt_score<NdtPoints>, c, pts_dev, n_dev, cap, T_dev, n_pose, neighbours, outlier_ratio, score_dev,
                              scratch_dev, stream);
}

int sps_ndt_top_poses(sps_ctx *c, const double *score_dev, const double *T_dev, int64_t n_pose, int min_corr, int k,
                      int32_t *top_index_dev, double *T_top_dev, int32_t *n_top_dev, void *stream) {
  if (!c || !score_dev || !T_dev || !top_index_dev || !T_top_dev || !n_top_dev) return fail(SPS_ERR_INVALID, "bad arguments");
  if (n_pose < 1 || n_pose > SPS_NDT_MAX_POSES) return fail(SPS_ERR_INVALID, "n_pose must be in [1, %d]", SPS_NDT_MAX_POSES);
  if (k < 1 || k > SPS_NDT_MAX_HYP) return fail(SPS_ERR_INVALID, "k must be in [1, %d]", SPS_NDT_MAX_HYP);
  HIP_TRY(hipSetDevice(c->device));
  hipLaunchKernelGGL(k_ndt_top, dim3(1), dim3(NDT_TOP_THREADS), 0, (hipStream_t)stream, score_dev, T_dev, (int)n_pose, min_corr, k,
                     top_index_dev, T_top_dev, n_top_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
