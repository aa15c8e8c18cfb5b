// ndt_pyramid_batch_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after
// ndt_d2d_host.inc.h): the coarse-to-fine NDT alignment from several start poses at once, of points and of source cells
// (ABI: the "NDT localiser, pyramid, several hypotheses" and "NDT localiser, distribution to distribution, pyramid, several
// hypotheses" sections of include/sps_hip.h; kernels: ndt_pyramid_batch_kernels.inc.h, and k_ndt_select of
// ndt_batch_kernels.inc.h for the selection).  Like sps_ndt_pyramid_align the calls neither allocate nor synchronise.

namespace {
// the batched coarse-to-fine alignment with the launches of one scan (k_ndt_pyr_assoc_batch / k_ndt_pyr_solve_batch /
// k_ndt_pyr_final_batch of NdtPoints: sps_ndt_pyramid_align_batch; of NdtCells: sps_ndt_pyramid_align_d2d_batch, whose
// elements are the levels' source records and whose n_dev holds two counts per level)
int ndt_pyramid_align_batch_impl(NdtPyrAssocBatchKernel assoc, NdtPyrSolveBatchKernel solve, NdtPyrFinalBatchKernel final_pass,
                                 sps_ctx *c, const double *elems_dev, const int32_t *n_dev, int64_t cap, const double *T_init_dev,
                                 int n_hyp, int iters, const int32_t *level_iters, int neighbours, int min_corr, double tol_t,
                                 double tol_r, double *T_out_dev, int32_t *status_dev, double *trace_dev, double *normal_dev,
                                 int32_t *level_dev, double *final_dev, int32_t *best_dev, double *T_best_dev, void *scratch_dev,
                                 void *stream) {
  if (!c || !n_dev || !T_init_dev || !level_iters || !T_out_dev || !status_dev || !final_dev || !best_dev || !T_best_dev ||
      !scratch_dev || cap < 0 || iters < 0 || (cap > 0 && !elems_dev) || (iters > 0 && (!trace_dev || !level_dev)))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (n_hyp < 1 || n_hyp > SPS_NDT_MAX_HYP) return fail(SPS_ERR_INVALID, "n_hyp must be in [1, %d]", SPS_NDT_MAX_HYP);
  const int L = c->ndt_pyr.n_levels;
  if (L < 1) return fail(SPS_ERR_INVALID, "sps_ndt_pyramid_build has not been called");
  if (int e = ndt_check_scan_limits(neighbours, cap, true, iters, tol_t, tol_r)) return e;
  NdtPyrCaps caps{};
  if (int e = ndt_pyr_caps(L, level_iters, caps)) return e;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)loc_align_blocks(cap);
  double *partial = (double *)scratch_dev;
  int *state = (int *)((char *)scratch_dev + ndt_batch_partial_bytes(cap, n_hyp));
  const int init_blocks = std::min(64, std::max(1, (iters * 28 + 255) / 256));
  hipLaunchKernelGGL(k_ndt_pyr_init_batch, dim3(init_blocks, n_hyp), dim3(256), 0, st, T_init_dev, n_hyp, iters, T_out_dev,
                     status_dev, state, trace_dev, normal_dev, level_dev);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(assoc, dim3(nb, n_hyp), dim3(256), 0, st, elems_dev, n_dev, (int)cap, c->ndt_pyr.dev, L, neighbours,
                       n_hyp, (const double *)T_out_dev, (const int *)state, partial);
    hipLaunchKernelGGL(solve, dim3(n_hyp), dim3(256), 0, st, (const double *)partial, nb, n_dev, (int)cap, it, iters, L, caps,
                       min_corr, tol_t, tol_r, n_hyp, T_init_dev, T_out_dev, status_dev, state, trace_dev, normal_dev, level_dev);
  }
  // every hypothesis once more at its final pose, against the scoring level whatever level it stopped at: the scores
  // k_ndt_select chooses by.  The pass finds that level on the device and leaves its count in hypothesis 0's spare state
  // word, by which the selection clips its rows.
  hipLaunchKernelGGL(final_pass, dim3(nb, n_hyp), dim3(256), 0, st, elems_dev, n_dev, (int)cap, c->ndt_pyr.dev, L, neighbours,
                     min_corr, n_hyp, (const double *)T_out_dev, state, partial);
  hipLaunchKernelGGL(k_ndt_select, dim3(1), dim3(256 * NDT_SELECT_GROUPS), 0, st, (const double *)partial, nb,
                     (const int *)state + NDT_PYR_FINAL_COUNT, (int)cap, n_hyp, min_corr, (const int *)status_dev,
                     (const double *)T_out_dev, T_init_dev, final_dev, best_dev, T_best_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
}  // namespace

// per hypothesis the partial rows of launch B (all hypotheses' rows first, the layout of sps_ndt_align_batch), then per
// hypothesis the state words
int64_t sps_ndt_pyramid_align_batch_scratch(int64_t cap, int n_hyp) {
  if (cap < 0 || cap > SPS_MAX_POINTS || n_hyp < 1 || n_hyp > SPS_NDT_MAX_HYP) return -1;
  return ndt_batch_partial_bytes(cap, n_hyp) + (int64_t)n_hyp * NDT_PYR_STATE * 4;
}

int sps_ndt_pyramid_align_batch(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_init_dev,
                                int n_hyp, int iters, const int32_t *level_iters, int neighbours, int min_corr, double tol_t,
                                double tol_r, double *T_out_dev, int32_t *status_dev, double *trace_dev, double *normal_dev,
                                int32_t *level_dev, double *final_dev, int32_t *best_dev, double *T_best_dev, void *scratch_dev,
                                void *stream) {
  return ndt_pyramid_align_batch_impl(k_ndt_pyr_assoc_batch<NdtPoints>, k_ndt_pyr_solve_batch<NdtPoints>,
                                      k_ndt_pyr_final_batch<NdtPoints>, c, pts_dev, n_dev, cap, T_init_dev, n_hyp, iters,
                                      level_iters, neighbours, min_corr, tol_t, tol_r, T_out_dev, status_dev, trace_dev,
                                      normal_dev, level_dev, final_dev, best_dev, T_best_dev, scratch_dev, stream);
}

// the point version's layout with the source capacity in place of the point capacity
int64_t sps_ndt_pyramid_align_d2d_batch_scratch(int64_t cap_src, int n_hyp) {
  return sps_ndt_pyramid_align_batch_scratch(cap_src, n_hyp);
}

int sps_ndt_pyramid_align_d2d_batch(sps_ctx *c, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src,
                                    const double *T_init_dev, int n_hyp, int iters, const int32_t *level_iters, int neighbours,
                                    int min_corr, double tol_t, double tol_r, double *T_out_dev, int32_t *status_dev,
                                    double *trace_dev, double *normal_dev, int32_t *level_dev, double *final_dev,
                                    int32_t *best_dev, double *T_best_dev, void *scratch_dev, void *stream) {
  return ndt_pyramid_align_batch_impl(k_ndt_pyr_assoc_batch<NdtCells>, k_ndt_pyr_solve_batch<NdtCells>,
                                      k_ndt_pyr_final_batch<NdtCells>, c, src_dev, n_src_dev, cap_src, T_init_dev, n_hyp, iters,
                                      level_iters, neighbours, min_corr, tol_t, tol_r, T_out_dev, status_dev, trace_dev,
                                      normal_dev, level_dev, final_dev, best_dev, T_best_dev, scratch_dev, stream);
}
