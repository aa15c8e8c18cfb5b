// loc_match_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace): the scan-matching status of a
// pose (host side: loc_match_host.inc.h; ABI: the "localiser, scan-matching status" section of include/sps_hip.h).
//
//   k_loc_match<W>      W lanes per scan point (SPS_LOC_MATCH_LANES = 64: one wave per point, as k_loc_assoc): valid?
//                       nearest map point (loc_nearest<W>, the search of k_loc_assoc), inlier?
//                       the workgroup adds its inliers' d2 in point order and counts valid points and inliers
//   k_loc_match_final   one workgroup: the workgroups' rows in loc_sum_rows' order, the two divisions, the verdict
//
// As the ICP: float64, every operation rounded on its own, no float atomics, no result that depends on arrival order.

#pragma clang fp contract(off)

struct LocMatchArgs {
  double md2, mr2;              // max_distance^2; max_range^2, < 0: no range limit
  double min_fraction, max_error;
  int min_valid;
};

#ifndef SPS_LOC_MATCH_LANES
// lanes per point of k_loc_match: 64, 32 or 16.  The results do not depend on it; 64 is the fastest of the three on 0.5 m and
// on 1 m cells (profiles/localiser_match/README.md)
#define SPS_LOC_MATCH_LANES 64
#endif

// a workgroup's row: its inliers' d2 added in point order, its valid points, its inliers.  A group of W lanes takes a
// point; groups of one wave work on different points, and every shuffle stays inside its group.
template <int W>
__global__ __launch_bounds__(256) void k_loc_match(const double *__restrict__ pts, const int *__restrict__ n_dev, int cap,
                                                    RadiusGrid g, const double *__restrict__ T, LocMatchArgs a,
                                                    double *__restrict__ d2_out, double *__restrict__ row_sum,
                                                    int *__restrict__ row_cnt) {
  __shared__ double d2s[LOC_PTS];
  __shared__ int flag[LOC_PTS];   // 0: no point or not valid, 1: valid, 3: valid and an inlier
  const int n = min(cap, max(*n_dev, 0));
  const int base = blockIdx.x * LOC_PTS;
  if (base >= n) return;
  const int lane = threadIdx.x % W, group = threadIdx.x / W;
  double R[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) R[i] = T[i];
  for (int k = group; k < LOC_PTS; k += 256 / W) {
    const int i = base + k;
    int f = 0;
    double d2 = 0.0;
    if (i < n) {
      const double px = pts[(size_t)i * 3], py = pts[(size_t)i * 3 + 1], pz = pts[(size_t)i * 3 + 2];
      const double range2 = loc_add(loc_add(loc_mul(px, px), loc_mul(py, py)), loc_mul(pz, pz));
      const bool valid = isfinite(px) && isfinite(py) && isfinite(pz) && (a.mr2 < 0.0 || range2 <= a.mr2);
      double out = -1.0;
      if (valid) {                                   // the same for every lane of the group
        double q[3];
        loc_transform(R, px, py, pz, q);
        double best;
        int best_j;
        loc_nearest<W>(g, q, a.md2, lane, best, best_j);
        f = 1, out = INFINITY;
        if (best_j != 0x7FFFFFFF) f = 3, d2 = best, out = best;
      }
      if (d2_out && lane == 0) d2_out[i] = out;
    }
    if (lane == 0) d2s[k] = d2, flag[k] = f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    int n_valid = 0, n_in = 0;
    for (int k = 0; k < LOC_PTS; ++k) {
      const int f = flag[k];
      if (f == 3) s = loc_add(s, d2s[k]);
      n_valid += f & 1, n_in += f >> 1;
    }
    row_sum[blockIdx.x] = s;
    row_cnt[2 * blockIdx.x] = n_valid, row_cnt[2 * blockIdx.x + 1] = n_in;
  }
}

// The rows of the ceil(n / LOC_PTS) workgroups that held points, as loc_sum_rows adds a column: LOC_SEG runs of
// consecutive rows, each in order, then the runs in order.  Thread 0 divides and decides.
//   out: double (inlier_fraction, matching_error, sum_d2, 0) | int32 (verdict, n_valid, n_inliers, n)
__global__ __launch_bounds__(64) void k_loc_match_final(const double *__restrict__ row_sum, const int *__restrict__ row_cnt,
                                                         const int *__restrict__ n_dev, int cap, const int *__restrict__ gate_in,
                                                         LocMatchArgs a, double *__restrict__ out) {
  __shared__ double seg[LOC_SEG];
  __shared__ int seg_cnt[LOC_SEG][2];
  const int n = min(cap, max(*n_dev, 0));
  const int nb = (n + LOC_PTS - 1) / LOC_PTS;
  const int t = threadIdx.x;
  if (t < LOC_SEG) {
    const int per = (nb + LOC_SEG - 1) / LOC_SEG;
    const int b1 = min(nb, (t + 1) * per);
    double s = 0.0;
    int n_valid = 0, n_in = 0;
    for (int b = t * per; b < b1; ++b) {
      s = loc_add(s, row_sum[b]);
      n_valid += row_cnt[2 * b], n_in += row_cnt[2 * b + 1];
    }
    seg[t] = s, seg_cnt[t][0] = n_valid, seg_cnt[t][1] = n_in;
  }
  __syncthreads();
  if (t != 0) return;
  double sum = 0.0;
  int n_valid = 0, n_in = 0;
  for (int i = 0; i < LOC_SEG; ++i) {
    sum = loc_add(sum, seg[i]);
    n_valid += seg_cnt[i][0], n_in += seg_cnt[i][1];
  }
  const double fraction = __ddiv_rn((double)n_in, (double)max(n_valid, 1));
  const double error = n_in > 0 ? __ddiv_rn(sum, (double)n_in) : INFINITY;
  const int gate = gate_in ? *gate_in : 0;
  int verdict = gate;
  if ((unsigned)gate <= 1u && !(n_valid >= a.min_valid && fraction >= a.min_fraction && error <= a.max_error))
    verdict = SPS_LOC_LOST;
  out[0] = fraction, out[1] = error, out[2] = sum, out[3] = 0.0;
  int *w = (int *)(out + 4);
  w[0] = verdict, w[1] = n_valid, w[2] = n_in, w[3] = n;
}

#pragma clang fp contract(fast)
