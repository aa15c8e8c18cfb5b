// sps_filter_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace): everything the reference's
// two SPS nodes do with the scores of a frame (c_ws/src/sps_filter/scripts/sps_node.py:123-161 and
// sps_node_cvm.py:145-184), in two launches (host side: sps_filter_finish in sps_hip.hip; ABI: the "streaming filter"
// section of include/sps_hip.h).
//
//   k_filter_count   pred = score < eps ? 0 : 1 (:131) -> labels and the debug cloud (x', y', z', pred) (:152-154); per
//                    workgroup the number of kept rows (block_sums) and, with a label column, one partial row of the
//                    metric accumulators count, TP, FP, FN, TN, sum (s-g)^2, sum g, sum g^2 (:123-134)
//   k_filter_write   order-preserving compaction of the WHOLE received rows that are kept (:148 / cvm :171), the submap
//                    debug cloud (vx, vy, vz, 1) (:157-161), and the partial rows combined in block order
//
// The kept rows go through the ordered compaction of aux_kernels.inc.h (k_filter_count fills block_sums from the ballot
// it shares with its confusion counters; k_filter_write places with compact_base / compact_rank).  No atomics anywhere:
// a position comes from the per-workgroup counts, a sum from the partial rows, both combined in a fixed order -- two runs on the same input give
// the same bits (unlike the f64 atomicAdds of k_metrics).

struct FilterFinishArgs {
  const float *scores;  // [n]
  int n;
  float eps;
  int strict;           // 0: keep score <= eps (sps_node.py:148); 1: keep score < eps, i.e. pred == 0 (sps_node_cvm.py:171)
  const float *raw;     // the scan rows as received, row stride ld, cols floats per row
  int64_t ld;
  int cols;
  int label_col;        // column of raw that holds the label, -1 = none
  const float *batch;   // sps_filter_prepare's rows: n x (0, x', y', z', 1) then n_sub x (0, vx, vy, vz, 0)
  const int *counts;    // sps_filter_prepare's counts: counts[0] = n_sub
  float *filtered;      // [., cols]  (each output may be null)
  int *count_out;
  int *labels;          // [n]
  float *cloud_tr;      // [n, 4]
  float *submap;        // [n_sub, 4]
  double *sums;         // [8]
  int *block_sums;      // [gridDim.x] kept rows per workgroup
  double *part;         // [gridDim.x][8] metric partial rows
};

__device__ inline bool filter_keep(float s, float eps, int strict) { return strict ? s < eps : s <= eps; }  // NaN: dropped

constexpr int FILTER_WAVES = SCAN_BLOCK / 64;

__global__ __launch_bounds__(SCAN_BLOCK) void k_filter_count(const FilterFinishArgs a) {
  __shared__ int cnt[5][FILTER_WAVES];      // kept, TP, FP, FN, TN per wave
  __shared__ double red[3][FILTER_WAVES];   // sum (s-g)^2, sum g, sum g^2 per wave
  const int p = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool in = p < a.n;
  const float s = in ? a.scores[p] : 0.f;
  const int pred = s < a.eps ? 0 : 1;  // NaN -> 1, as np.where(s < eps, 0, 1)
  const bool keep = in && filter_keep(s, a.eps, a.strict);
  if (in) {
    if (a.labels) a.labels[p] = pred;
    if (a.cloud_tr) {
      const float *r = a.batch + (size_t)p * 5;
      float *o = a.cloud_tr + (size_t)p * 4;
      o[0] = r[1];
      o[1] = r[2];
      o[2] = r[3];
      o[3] = (float)pred;
    }
  }
  const bool metrics = a.label_col >= 0;
  int gt = -1;
  double v[3] = {0.0, 0.0, 0.0};
  if (metrics && in) {
    const float g = a.raw[(size_t)p * a.ld + a.label_col];
    gt = g < a.eps ? 0 : 1;
    const double d = (double)s - (double)g;
    v[0] = d * d;
    v[1] = (double)g;
    v[2] = (double)g * (double)g;
  }
  const unsigned long long bk = __ballot(keep);
  const unsigned long long b1 = __ballot(gt == 1 && pred == 1), b2 = __ballot(gt == 0 && pred == 1);
  const unsigned long long b3 = __ballot(gt == 1 && pred == 0), b4 = __ballot(gt == 0 && pred == 0);
  if (metrics) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_down(v[j], o, 64);  // a fixed tree: the same bits every run
  }
  if (lane == 0) {
    cnt[0][wave] = __popcll(bk);
    cnt[1][wave] = __popcll(b1);
    cnt[2][wave] = __popcll(b2);
    cnt[3][wave] = __popcll(b3);
    cnt[4][wave] = __popcll(b4);
    red[0][wave] = v[0];
    red[1][wave] = v[1];
    red[2][wave] = v[2];
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j == 0) {
    int tot = 0;
    for (int i = 0; i < FILTER_WAVES; ++i) tot += cnt[0][i];
    a.block_sums[blockIdx.x] = tot;
  }
  if (metrics && j < 8) {
    double x = 0.0;
    if (j == 0) x = (double)max(0, min(SCAN_BLOCK, a.n - (int)blockIdx.x * SCAN_BLOCK));
    else if (j < 5) {
      int t = 0;
      for (int i = 0; i < FILTER_WAVES; ++i) t += cnt[j][i];
      x = (double)t;
    } else
      for (int i = 0; i < FILTER_WAVES; ++i) x += red[j - 5][i];  // waves in order
    a.part[(size_t)blockIdx.x * 8 + j] = x;
  }
}

constexpr int FILTER_SLICES = 32;  // k_filter_write combines the partial rows as 32 interleaved slices, then the slices in order

__global__ __launch_bounds__(SCAN_BLOCK) void k_filter_write(const FilterFinishArgs a) {
  __shared__ int lds[FILTER_WAVES];
  __shared__ int wave_off[FILTER_WAVES];
  __shared__ double sl[FILTER_SLICES][8];
  const int p = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  if (a.filtered) {
    const int base = compact_base(a.block_sums, lds);
    const bool keep = p < a.n && filter_keep(a.scores[p], a.eps, a.strict);
    int kept;
    const int k = compact_rank(base, keep, wave_off, kept);
    if (keep) {
      const float *r = a.raw + (size_t)p * a.ld;
      float *o = a.filtered + (size_t)k * a.cols;
      for (int j = 0; j < a.cols; ++j) o[j] = r[j];
    }
    if (compact_last_thread()) *a.count_out = kept;
  }
  if (a.submap) {
    const int n_sub = min(a.n, a.counts[0]);  // (the submap never has more rows than the scan; the clamp bounds the reads)
    if (p < n_sub) {
      const float *r = a.batch + (size_t)(a.n + p) * 5;
      float *o = a.submap + (size_t)p * 4;
      o[0] = r[1];
      o[1] = r[2];
      o[2] = r[3];
      o[3] = 1.f;  // submap_labels = torch.ones (sps_node.py:158)
    }
  }
  if (a.sums && a.label_col >= 0 && blockIdx.x == 0) {
    const int t = threadIdx.x;
    if (t < FILTER_SLICES * 8) {
      const int j = t & 7, k = t >> 3;
      double x = 0.0;
      for (int b = k; b < (int)gridDim.x; b += FILTER_SLICES) x += a.part[(size_t)b * 8 + j];
      sl[k][j] = x;
    }
    __syncthreads();
    if (t < 8) {
      double x = 0.0;
      for (int k = 0; k < FILTER_SLICES; ++k) x += sl[k][t];
      a.sums[t] = x;
    }
  }
}
