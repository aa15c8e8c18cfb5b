// ndt_batch_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_host.inc.h): the NDT
// localiser from several start poses at once (ABI: the "NDT localiser, several hypotheses" section of include/sps_hip.h;
// kernels: ndt_batch_kernels.inc.h).  Like sps_ndt_align the call neither allocates nor synchronises.

namespace {
inline int64_t ndt_batch_partial_bytes(int64_t cap, int n_hyp) { return (int64_t)n_hyp * loc_align_blocks(cap) * LOC_TERMS * 8; }

// the batch on the single map with launch A `assoc` (k_ndt_assoc_batch of NdtPoints: sps_ndt_align_batch; of NdtCells:
// sps_ndt_align_d2d_batch)
int ndt_align_batch_impl(NdtAssocBatchKernel assoc, sps_ctx *c, const double *elems_dev, const int32_t *n_dev, int64_t cap,
                         const double *T_init_dev, int n_hyp, int iters, int neighbours, int min_corr, double outlier_ratio,
                         double tol_t, double tol_r, double *T_out_dev, int32_t *status_dev, double *trace_dev,
                         double *normal_dev, double *final_dev, int32_t *best_dev, double *T_best_dev, void *scratch_dev,
                         void *stream) {
  if (!c || !n_dev || !T_init_dev || !T_out_dev || !status_dev || !final_dev || !best_dev || !T_best_dev || !scratch_dev ||
      cap < 0 || iters < 0 || (cap > 0 && !elems_dev) || (iters > 0 && !trace_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (n_hyp < 1 || n_hyp > SPS_NDT_MAX_HYP) return fail(SPS_ERR_INVALID, "n_hyp must be in [1, %d]", SPS_NDT_MAX_HYP);
  NdtGauss gs;
  if (int e = ndt_check_scan_args(c, neighbours, cap, outlier_ratio, gs, true, iters, tol_t, tol_r)) return e;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)loc_align_blocks(cap);
  double *partial = (double *)scratch_dev;
  int *done = (int *)((char *)scratch_dev + ndt_batch_partial_bytes(cap, n_hyp));
  if (iters > 0) HIP_TRY(hipMemsetAsync(trace_dev, 0, (size_t)n_hyp * iters * 4 * sizeof(double), st));
  if (iters > 0 && normal_dev) HIP_TRY(hipMemsetAsync(normal_dev, 0, (size_t)n_hyp * iters * 28 * sizeof(double), st));
  hipLaunchKernelGGL(k_loc_init_batch, dim3(n_hyp), dim3(64), 0, st, T_init_dev, n_hyp, T_out_dev, status_dev, done);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(assoc, dim3(nb, n_hyp), dim3(256), 0, st, elems_dev, n_dev, (int)cap, c->ndt_map.lv[0].m,
                       gs, neighbours, n_hyp, (const double *)T_out_dev, (const int *)done, 0, partial);
    hipLaunchKernelGGL(k_loc_solve_batch, dim3(n_hyp), dim3(256), 0, st, (const double *)partial, nb, n_dev, (int)cap, it, iters,
                       min_corr, tol_t, tol_r, n_hyp, T_init_dev, T_out_dev, status_dev, done, trace_dev, normal_dev);
  }
  // every hypothesis once more at its final pose: the scores k_ndt_select chooses by
  hipLaunchKernelGGL(assoc, dim3(nb, n_hyp), dim3(256), 0, st, elems_dev, n_dev, (int)cap, c->ndt_map.lv[0].m,
                     gs, neighbours, n_hyp, (const double *)T_out_dev, (const int *)done, 1, partial);
  hipLaunchKernelGGL(k_ndt_select, dim3(1), dim3(256 * NDT_SELECT_GROUPS), 0, st, (const double *)partial, nb, n_dev, (int)cap,
                     n_hyp, min_corr, (const int *)status_dev, (const double *)T_out_dev, T_init_dev, final_dev, best_dev,
                     T_best_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
}  // namespace

// the partial rows of every hypothesis, then one done flag each
int64_t sps_ndt_align_batch_scratch(int64_t cap, int n_hyp) {
  if (cap < 0 || cap > SPS_MAX_POINTS || n_hyp < 1 || n_hyp > SPS_NDT_MAX_HYP) return -1;
  return ndt_batch_partial_bytes(cap, n_hyp) + (((int64_t)n_hyp * 4 + 15) / 16) * 16;
}

int sps_ndt_align_batch(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_init_dev, int n_hyp,
                        int iters, int neighbours, int min_corr, double outlier_ratio, double tol_t, double tol_r,
                        double *T_out_dev, int32_t *status_dev, double *trace_dev, double *normal_dev, double *final_dev,
                        int32_t *best_dev, double *T_best_dev, void *scratch_dev, void *stream) {
  return ndt_align_batch_impl(k_ndt_assoc_batch<NdtPoints>, c, pts_dev, n_dev, cap, T_init_dev, n_hyp, iters, neighbours, min_corr,
                              outlier_ratio, tol_t, tol_r, T_out_dev, status_dev, trace_dev, normal_dev, final_dev, best_dev,
                              T_best_dev, scratch_dev, stream);
}
