// ndt_d2d_batch_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_d2d_host.inc.h):
// distribution-to-distribution NDT from several start poses at once, and the D2D score of many poses (ABI: the "NDT
// localiser, distribution to distribution, several poses" section of include/sps_hip.h; kernels:
// ndt_d2d_batch_kernels.inc.h).  The layouts of the scratch are those of sps_ndt_align_batch and sps_ndt_score_poses with
// the source capacity in place of the point capacity.  Neither call allocates or synchronises.

int64_t sps_ndt_align_d2d_batch_scratch(int64_t cap_src, int n_hyp) { return sps_ndt_align_batch_scratch(cap_src, n_hyp); }

int sps_ndt_align_d2d_batch(sps_ctx *c, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src, const double *T_init_dev,
                            int n_hyp, int iters, int neighbours, int min_corr, double outlier_ratio, double tol_t, double tol_r,
                            double *T_out_dev, int32_t *status_dev, double *trace_dev, double *normal_dev, double *final_dev,
                            int32_t *best_dev, double *T_best_dev, void *scratch_dev, void *stream) {
  if (!c || !n_src_dev || !T_init_dev || !T_out_dev || !status_dev || !final_dev || !best_dev || !T_best_dev || !scratch_dev ||
      cap_src < 0 || iters < 0 || (cap_src > 0 && !src_dev) || (iters > 0 && !trace_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (n_hyp < 1 || n_hyp > SPS_NDT_MAX_HYP) return fail(SPS_ERR_INVALID, "n_hyp must be in [1, %d]", SPS_NDT_MAX_HYP);
  NdtGauss gs;
  if (int e = ndt_check_scan_args(c, neighbours, cap_src, outlier_ratio, gs, true, iters, tol_t, tol_r)) return e;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)loc_align_blocks(cap_src);
  double *partial = (double *)scratch_dev;
  int *done = (int *)((char *)scratch_dev + ndt_batch_partial_bytes(cap_src, n_hyp));
  if (iters > 0) HIP_TRY(hipMemsetAsync(trace_dev, 0, (size_t)n_hyp * iters * 4 * sizeof(double), st));
  if (iters > 0 && normal_dev) HIP_TRY(hipMemsetAsync(normal_dev, 0, (size_t)n_hyp * iters * 28 * sizeof(double), st));
  hipLaunchKernelGGL(k_loc_init_batch, dim3(n_hyp), dim3(64), 0, st, T_init_dev, n_hyp, T_out_dev, status_dev, done);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(k_ndt_d2d_assoc_batch, dim3(nb, n_hyp), dim3(256), 0, st, src_dev, n_src_dev, (int)cap_src,
                       c->ndt_map.lv[0].m, gs, neighbours, n_hyp, (const double *)T_out_dev, (const int *)done, 0, partial);
    hipLaunchKernelGGL(k_loc_solve_batch, dim3(n_hyp), dim3(256), 0, st, (const double *)partial, nb, n_src_dev, (int)cap_src, it,
                       iters, min_corr, tol_t, tol_r, n_hyp, T_init_dev, T_out_dev, status_dev, done, trace_dev, normal_dev);
  }
  // every hypothesis once more at its final pose: the scores k_ndt_select chooses by
  hipLaunchKernelGGL(k_ndt_d2d_assoc_batch, dim3(nb, n_hyp), dim3(256), 0, st, src_dev, n_src_dev, (int)cap_src, c->ndt_map.lv[0].m,
                     gs, neighbours, n_hyp, (const double *)T_out_dev, (const int *)done, 1, partial);
  hipLaunchKernelGGL(k_ndt_select, dim3(1), dim3(256 * NDT_SELECT_GROUPS), 0, st, (const double *)partial, nb, n_src_dev,
                     (int)cap_src, n_hyp, min_corr, (const int *)status_dev, (const double *)T_out_dev, T_init_dev, final_dev,
                     best_dev, T_best_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int64_t sps_ndt_score_d2d_scratch(int64_t cap_src, int64_t n_pose) { return sps_ndt_score_scratch(cap_src, n_pose); }

int sps_ndt_score_poses_d2d(sps_ctx *c, const double *src_dev, const int32_t *n_src_dev, int64_t cap_src, const double *T_dev,
                            int64_t n_pose, int neighbours, double outlier_ratio, double *score_dev, void *scratch_dev,
                            void *stream) {
  if (!c || !n_src_dev || !T_dev || !score_dev || !scratch_dev || cap_src < 0 || (cap_src > 0 && !src_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (n_pose < 1 || n_pose > SPS_NDT_MAX_POSES) return fail(SPS_ERR_INVALID, "n_pose must be in [1, %d]", SPS_NDT_MAX_POSES);
  NdtGauss gs;
  if (int e = ndt_check_scan_args(c, neighbours, cap_src, outlier_ratio, gs, false)) return e;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)loc_align_blocks(cap_src);
  const int64_t chunk = ndt_score_chunk(cap_src, n_pose);
  double *partial = (double *)scratch_dev;
  for (int64_t p0 = 0; p0 < n_pose; p0 += chunk) {      // chunks follow one another on the stream and share the scratch
    const int np = (int)std::min(chunk, n_pose - p0);
    hipLaunchKernelGGL(k_ndt_d2d_score, dim3(nb, (np + NDT_SCORE_TILE - 1) / NDT_SCORE_TILE), dim3(256), 0, st, src_dev,
                       n_src_dev, (int)cap_src, c->ndt_map.lv[0].m, gs, neighbours, T_dev + p0 * 16, np, partial);
    hipLaunchKernelGGL(k_ndt_score_reduce, dim3((np + NDT_REDUCE_POSES - 1) / NDT_REDUCE_POSES), dim3(256), 0, st,
                       (const double *)partial, nb, n_src_dev, (int)cap_src, np, score_dev + p0 * 2);
  }
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
