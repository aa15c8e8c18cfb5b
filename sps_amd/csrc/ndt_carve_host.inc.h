// ndt_carve_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block, after ndt_update_host.inc.h): free-space
// carving of the online NDT map (ABI: the "NDT localiser, online map: free-space carving" section of include/sps_hip.h;
// kernels: ndt_carve_kernels.inc.h).  sps_ndt_map_carve neither allocates nor synchronises; its three per-cell arrays belong
// to the dynamic map (ndt_map_make, ndt_host.inc.h) and it needs no scratch of the caller's.

int64_t sps_ndt_map_carve_scratch(int64_t cap) {
  if (cap < 0 || cap > SPS_NDT_UPDATE_MAX_POINTS) return -1;
  return 0;
}

int sps_ndt_map_carve(sps_ctx *c, const double *pts_dev, const int32_t *n_dev, int64_t cap, const double *T_host,
                      const double *T_dev, const int32_t *gate_dev, double end_margin, double through_sigma, int min_pass,
                      int miss_frames, int max_steps, int32_t *info_dev, void *scratch_dev, void *stream) {
  (void)scratch_dev;   // sps_ndt_map_carve_scratch is 0
  if (!c || !n_dev || !info_dev || cap < 0 || (cap > 0 && !pts_dev) || (!T_host && !T_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (!c->ndt.h.keys || c->ndt_dyn.capacity <= 0)
    return fail(SPS_ERR_INVALID, "the map of this context is not dynamic (sps_ndt_map_build_dynamic)");
  if (cap > SPS_NDT_UPDATE_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_NDT_UPDATE_MAX_POINTS);
  if (!(end_margin >= 0.0) || std::isinf(end_margin)) return fail(SPS_ERR_INVALID, "end_margin must be finite and >= 0");
  if (!(through_sigma > 0.0) || std::isinf(through_sigma)) return fail(SPS_ERR_INVALID, "through_sigma must be finite and > 0");
  if (min_pass < 1 || miss_frames < 1) return fail(SPS_ERR_INVALID, "min_pass and miss_frames must be >= 1");
  if (max_steps < 1 || max_steps > 4096) return fail(SPS_ERR_INVALID, "max_steps must be in [1, 4096]");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  LocPose Th{};
  if (T_host)
    for (int i = 0; i < 16; ++i) Th.m[i] = T_host[i];
  const NdtDyn &d = c->ndt_dyn;
  const NdtCarveParams p{end_margin, through_sigma * through_sigma, min_pass, miss_frames, max_steps};
  const int nbp = (int)((cap + 255) / 256 > 0 ? (cap + 255) / 256 : 1);
  const int nbc = (d.capacity + 255) / 256;
  hipLaunchKernelGGL(k_ndt_carve_begin, dim3(nbc), dim3(256), 0, st, gate_dev, d, info_dev);
  hipLaunchKernelGGL(k_ndt_carve_rays, dim3(nbp), dim3(256), 0, st, pts_dev, n_dev, (int)cap, Th, T_dev, gate_dev, c->ndt, d, p,
                     info_dev);
  hipLaunchKernelGGL(k_ndt_carve_decide, dim3(nbc), dim3(256), 0, st, gate_dev, d, p, info_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int sps_ndt_map_carve_cells(sps_ctx *c, int32_t *pass_out_dev, int32_t *hit_out_dev, int32_t *miss_out_dev) {
  if (!c) return fail(SPS_ERR_INVALID, "ctx is null");
  if (!c->ndt.h.keys || c->ndt_dyn.capacity <= 0)
    return fail(SPS_ERR_INVALID, "the map of this context is not dynamic (sps_ndt_map_build_dynamic)");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t bytes = (size_t)c->ndt_dyn.capacity * sizeof(int32_t);
  if (pass_out_dev) HIP_TRY(hipMemcpy(pass_out_dev, c->ndt_dyn.pass, bytes, hipMemcpyDeviceToDevice));
  if (hit_out_dev) HIP_TRY(hipMemcpy(hit_out_dev, c->ndt_dyn.hit, bytes, hipMemcpyDeviceToDevice));
  if (miss_out_dev) HIP_TRY(hipMemcpy(miss_out_dev, c->ndt_dyn.miss, bytes, hipMemcpyDeviceToDevice));
  HIP_TRY(hipDeviceSynchronize());
  return SPS_OK;
}
