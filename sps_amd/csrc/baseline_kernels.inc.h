// baseline_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace): the per-frame pieces of the
// reference's 4DMOS and MapMOS nodes around the head forward (host side: baseline_host.inc.h; ABI: the "online baseline
// filters" section of include/sps_hip.h).  The scan / window rows themselves are written by k_transform_points<.., true>
// (aux_kernels.inc.h) with the node's time stamp and per-row feature.
//
//   k_crop_count / k_crop_write   mapmos_node.py:63-68, 79-80  select_points_within_radius (np.where order)
//   k_label_count / k_label_write mos4d_node.py:121-127, mapmos_node.py:98-103  logits > 0, filter label 0, confusion counts
//
// Both are pairs of the ordered compaction (compact_count / compact_base / compact_rank, aux_kernels.inc.h): no atomics
// decide an output position, so the outputs keep the input order.

// mapmos_node.py:63-68: sqrt(sum((p - c) ** 2, axis=1)) <= r in float64.  numpy adds the three squares left to right;
// every operation is rounded on its own (no contraction into FMA), so the kept set is the reference's bit for bit,
// points on the sphere included.  NaN coordinates are never kept (NaN <= r is false).
template <typename TIN>
__device__ inline bool crop_keep(const TIN *__restrict__ map, int64_t ld, int i, double cx, double cy, double cz, double r) {
  const TIN *p = map + (size_t)i * ld;
  const double dx = __dadd_rn((double)p[0], -cx), dy = __dadd_rn((double)p[1], -cy), dz = __dadd_rn((double)p[2], -cz);
  const double s = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
  return __dsqrt_rn(s) <= r;
}

template <typename TIN>
__global__ __launch_bounds__(SCAN_BLOCK) void k_crop_count(const TIN *__restrict__ map, int64_t ld, int m, double cx, double cy,
                                                            double cz, double r, int *__restrict__ block_sums) {
  __shared__ int lds[SCAN_BLOCK / 64];
  const int p = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  compact_count(p < m && crop_keep(map, ld, p, cx, cy, cz, r), lds, block_sums);
}

// The kept map point of rank k (ascending map index) becomes row n_scan + k of the batch: (0, x, y, z, -1) as float32
// (mapmos.py:39-47, map t = -1) and feat_out[n_scan + k] = feat_value.  Ranks >= cap are dropped: counts[0] = min(kept,
// cap), counts[1] = n_scan + counts[0], and error bit 32 (sps_check: SPS_ERR_ITEMCAP) is raised when kept > cap.
template <typename TIN>
__global__ __launch_bounds__(SCAN_BLOCK) void k_crop_write(const TIN *__restrict__ map, int64_t ld, int m, double cx, double cy,
                                                            double cz, double r, const int *__restrict__ block_sums,
                                                            float *__restrict__ rows, int64_t ldo, int n_scan, int cap,
                                                            float *__restrict__ feat_out, float feat_value,
                                                            int *__restrict__ counts, int *__restrict__ err) {
  __shared__ int lds[SCAN_BLOCK / 64];
  __shared__ int wave_off[SCAN_BLOCK / 64];
  const int base = compact_base(block_sums, lds);
  const int p = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  const int flag = p < m && crop_keep(map, ld, p, cx, cy, cz, r);
  int kept;
  const int k = compact_rank(base, flag, wave_off, kept);
  if (flag && k < cap) {
    const TIN *s = map + (size_t)p * ld;
    float *o = rows + (size_t)(n_scan + k) * ldo;
    o[0] = 0.f;
    o[1] = (float)s[0];
    o[2] = (float)s[1];
    o[3] = (float)s[2];
    o[4] = -1.f;
    if (feat_out) feat_out[n_scan + k] = feat_value;
  }
  if (compact_last_thread()) {
    counts[0] = min(kept, cap);
    counts[1] = n_scan + min(kept, cap);
    if (kept > cap) atomicOr(err, 32);
  }
}

// to_label (mapmos.py:84-89; mos4d_node.py:121: `> 0`): label = logit > 0 (NaN -> 0).  labels[p] in {0, 1} as float32;
// with a ground-truth column (mos4d_node.py:83: gt = s < 0.84 ? 0 : 1, float32 compare) the confusion counts of
// util.calculate_metrics (positive = 1) are added to conf[0..3] = TP, FP, FN, TN -- integer atomics, one per workgroup
// and counter, so the counts do not depend on the arrival order.
__global__ __launch_bounds__(SCAN_BLOCK) void k_label_count(const float *__restrict__ logits, int64_t ldl, int n,
                                                             const float *__restrict__ gt, int64_t ldg, float gt_eps,
                                                             float *__restrict__ labels, int *__restrict__ block_sums,
                                                             int *__restrict__ conf) {
  __shared__ int lds[SCAN_BLOCK / 64];
  const int p = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  int pred = 0;
  if (p < n) {
    pred = logits[(size_t)p * ldl] > 0.f ? 1 : 0;
    labels[p] = pred ? 1.f : 0.f;
  }
  compact_count(p < n && !pred, lds, block_sums);
  if (gt) {
    const int g = p < n ? (gt[(size_t)p * ldg] < gt_eps ? 0 : 1) : -1;
    const int tp = block_reduce_sum(g == 1 && pred == 1, lds);
    const int fp = block_reduce_sum(g == 0 && pred == 1, lds);
    const int fn = block_reduce_sum(g == 1 && pred == 0, lds);
    const int tn = block_reduce_sum(g == 0 && pred == 0, lds);
    if (threadIdx.x == 0) {
      if (tp) atomicAdd(conf + 0, tp);
      if (fp) atomicAdd(conf + 1, fp);
      if (fn) atomicAdd(conf + 2, fn);
      if (tn) atomicAdd(conf + 3, tn);
    }
  }
}

// `scan[scan_labels == 0]` with the label column (mos4d_node.py:124-127, mapmos_node.py:100-101): the first three floats of
// every row whose label is 0, in input order, as out rows (x, y, z, 0); *count_out = rows kept.
__global__ __launch_bounds__(SCAN_BLOCK) void k_label_write(const float *__restrict__ logits, int64_t ldl, int n,
                                                             const int *__restrict__ block_sums, const float *__restrict__ rows,
                                                             int64_t ld, float *__restrict__ out, int *__restrict__ count_out) {
  __shared__ int lds[SCAN_BLOCK / 64];
  __shared__ int wave_off[SCAN_BLOCK / 64];
  const int base = compact_base(block_sums, lds);
  const int p = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  const int flag = p < n && !(logits[(size_t)p * ldl] > 0.f);
  int kept;
  const int k = compact_rank(base, flag, wave_off, kept);
  if (flag) {
    const float *r = rows + (size_t)p * ld;
    float *o = out + (size_t)k * 4;
    o[0] = r[0];
    o[1] = r[1];
    o[2] = r[2];
    o[3] = 0.f;
  }
  if (compact_last_thread()) *count_out = kept;
}
