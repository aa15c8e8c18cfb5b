// baseline_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block): the entry points of the online
// 4DMOS / MapMOS / mask filters (ABI: the "online baseline filters" section of include/sps_hip.h; kernels:
// baseline_kernels.inc.h and k_transform_points).  None of them synchronises with the host.

static_assert(SPS_CROP_BLOCK == SCAN_BLOCK, "sps_radius_crop's scratch holds one int per SCAN_BLOCK map rows");

int sps_forward_head_n(sps_ctx *c, const float *coords, int64_t ld, int64_t n_max, const int32_t *n_dev, float vs,
                       const float *feats, float t_base, float *out, int64_t ldo, int activation, void *stream) {
  if (!n_dev) return fail(SPS_ERR_INVALID, "n_dev is null");
  if (c && c->have_weights && ldo < c->net->out_channels) return fail(SPS_ERR_INVALID, "ldo is smaller than out_channels");
  if (activation != 0 && activation != 1) return fail(SPS_ERR_INVALID, "activation must be 0 (none) or 1 (sigmoid)");
  if (!(t_base == floorf(t_base)) || fabsf(t_base) > 16777216.f) return fail(SPS_ERR_INVALID, "t_base must be an integer");
  ForwardOpts fo;
  fo.head = true;
  fo.feats = n_max > 0 ? feats : nullptr;
  fo.t_base = t_base;
  fo.ldo = ldo;
  fo.act = activation;
  fo.n_dev = n_dev;
  return forward_impl(c, coords, ld, n_max, vs, out, fo, stream);
}

int sps_transform_rows(sps_ctx *c, const void *xyz_dev, int in_f64, int64_t ld, int64_t n, const double *T_host, float t,
                       float *rows_dev, int64_t ldo, float *feat_dev, float feat_value, void *stream) {
  if (!(t == floorf(t))) return fail(SPS_ERR_INVALID, "t must be an integer");
  RowWrite rw;
  rw.t = t;
  rw.feat = feat_dev;
  rw.feat_value = feat_value;
  return transform_impl(c, xyz_dev, in_f64, ld, n, T_host, rows_dev, 0, true, ldo, stream, rw);
}

int sps_transform_points_n(sps_ctx *c, const void *xyz_dev, int in_f64, int64_t ld, int64_t n_max, const int32_t *n_dev,
                           const double *T_host, void *out_dev, int out_f64, int64_t ldo, void *stream) {
  if (!n_dev) return fail(SPS_ERR_INVALID, "n_dev is null");
  RowWrite rw;
  rw.n_dev = n_dev;
  return transform_impl(c, xyz_dev, in_f64, ld, n_max, T_host, out_dev, out_f64, false, ldo, stream, rw);
}

int sps_radius_crop(sps_ctx *c, const void *map_dev, int in_f64, int64_t ld, int64_t m, const double *T_host, double r,
                    int32_t *scratch_dev, int64_t n_scan, float *rows_dev, int64_t ldo, int64_t cap, float *feat_dev,
                    float feat_value, int32_t *counts_dev, void *stream) {
  if (!c || !counts_dev || !scratch_dev || m < 0 || ld < 3 || ldo < 5 || n_scan < 0 || cap < 0 || (m > 0 && !map_dev) ||
      (cap > 0 && !rows_dev))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (!(r >= 0.0) || std::isinf(r)) return fail(SPS_ERR_INVALID, "radius must be finite and >= 0");
  if (m > SPS_MAX_POINTS || n_scan + cap > SPS_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_MAX_POINTS);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  // mapmos_node.py:79: origin = T[:3, 3]
  const double cx = T_host ? T_host[3] : 0.0, cy = T_host ? T_host[7] : 0.0, cz = T_host ? T_host[11] : 0.0;
  // an empty map still runs one (empty) workgroup: it publishes counts = [0, n_scan]
  const int nb = (int)std::max<int64_t>(1, (m + SCAN_BLOCK - 1) / SCAN_BLOCK);
  if (in_f64) {
    hipLaunchKernelGGL(k_crop_count<double>, dim3(nb), dim3(SCAN_BLOCK), 0, st, (const double *)map_dev, ld, (int)m, cx, cy, cz,
                       r, scratch_dev);
    hipLaunchKernelGGL(k_crop_write<double>, dim3(nb), dim3(SCAN_BLOCK), 0, st, (const double *)map_dev, ld, (int)m, cx, cy, cz,
                       r, scratch_dev, rows_dev, ldo, (int)n_scan, (int)cap, feat_dev, feat_value, counts_dev, c->err);
  } else {
    hipLaunchKernelGGL(k_crop_count<float>, dim3(nb), dim3(SCAN_BLOCK), 0, st, (const float *)map_dev, ld, (int)m, cx, cy, cz,
                       r, scratch_dev);
    hipLaunchKernelGGL(k_crop_write<float>, dim3(nb), dim3(SCAN_BLOCK), 0, st, (const float *)map_dev, ld, (int)m, cx, cy, cz,
                       r, scratch_dev, rows_dev, ldo, (int)n_scan, (int)cap, feat_dev, feat_value, counts_dev, c->err);
  }
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int sps_label_filter(sps_ctx *c, const float *logits_dev, int64_t ld_logits, int64_t n, const float *rows_dev, int64_t ld,
                     const float *gt_dev, int64_t ld_gt, float *labels_dev, float *out_dev, int32_t *counts_dev, void *stream) {
  if (!c || !counts_dev || n < 0 || ld_logits < 1 || ld < 3 || (gt_dev && ld_gt < 1) ||
      (n > 0 && (!logits_dev || !rows_dev || !labels_dev || !out_dev)))
    return fail(SPS_ERR_INVALID, "bad arguments");
  if (n > SPS_MAX_POINTS) return fail(SPS_ERR_INVALID, "too many points (limit %d)", SPS_MAX_POINTS);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(counts_dev, 0, 5 * sizeof(int32_t), st));
  if (n == 0) return SPS_OK;
  if (n > c->cap) {
    int rc = reserve(c, n);
    if (rc != SPS_OK) return rc;
  }
  const int nb = (int)((n + SCAN_BLOCK - 1) / SCAN_BLOCK);
  hipLaunchKernelGGL(k_label_count, dim3(nb), dim3(SCAN_BLOCK), 0, st, logits_dev, ld_logits, (int)n, gt_dev, ld_gt, 0.84f,
                     labels_dev, c->block_sums, counts_dev + 1);
  hipLaunchKernelGGL(k_label_write, dim3(nb), dim3(SCAN_BLOCK), 0, st, logits_dev, ld_logits, (int)n, c->block_sums, rows_dev,
                     ld, out_dev, counts_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
