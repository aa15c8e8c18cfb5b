// ndt_search_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after
// ndt_batch_kernels.inc.h): the NDT score of many poses and the choice of the best of them (host side:
// ndt_search_host.inc.h; ABI: the "NDT localiser, pose search" section of include/sps_hip.h).
//
//   k_ndt_score          grid (element blocks, pose tiles): partial[pose][block] = (score, elements counted) of the
//                        block's LOC_PTS elements of the scan at every pose of the tile; a template over the scan (NdtPoints
//                        of ndt_kernels.inc.h, NdtCells of ndt_d2d_kernels.inc.h), as k_ndt_assoc
//   k_ndt_score_reduce   score[pose] = the blocks of the pose added in loc_sum_rows' order
//   k_ndt_top            one workgroup: the K best poses by (score descending, index ascending)
//
// Per element and pose k_ndt_score calls what phase 1 of ndt_assoc_body calls (Scan::hit), and of the 29 terms only the
// score (27) and the count (28) are formed; the sums run in the orders of ndt_assoc_reduce and loc_sum_rows, so score[pose]
// has the bits of final_dev[k] of sps_ndt_align_batch(iters = 0), or of sps_ndt_align_d2d_batch, started at that pose.
// Everything is float64, every operation is rounded on its own, stores are plain vector stores, nothing is atomic.

#pragma clang fp contract(off)

constexpr int NDT_SCORE_TILE = 32;      // poses of one workgroup of k_ndt_score (held in LDS, 12 doubles each)
constexpr int NDT_REDUCE_POSES = 16;    // poses of one workgroup of k_ndt_score_reduce (LOC_SEG x 2 threads each)
constexpr int NDT_TOP_THREADS = 1024;
static_assert(NDT_REDUCE_POSES * LOC_SEG * 2 == 256, "k_ndt_score_reduce: one workgroup of 256");

// NDT_LANES lanes per element of the scan (a point, a source cell), LOC_PTS elements per workgroup, as in k_ndt_assoc.  The
// workgroup reads its elements once and walks the poses of its tile: lane c < neighbours looks up cell c of the element's
// place at the pose (Scan::hit), the element's lane 0 adds the contributing cells in lookup order; then thread j adds the
// LOC_PTS elements of pose j in index order.  An element that is not valid (Scan::valid: a source cell's flag) adds 0
// and is not counted, which is what its row of zero terms adds in ndt_assoc_body.
// nb = gridDim.x = the partial rows of one pose.  The +1 pads keep the last step free of LDS bank conflicts.
template <class Scan>
__global__ __launch_bounds__(256) void k_ndt_score(const double *__restrict__ elems, const int *__restrict__ n_dev, int cap,
                                                    NdtMap m, NdtGauss gs, int neighbours, const double *__restrict__ T,
                                                    int n_pose, double *__restrict__ partial) {
  __shared__ double pose[NDT_SCORE_TILE][12];
  __shared__ double sc[NDT_SCORE_TILE][LOC_PTS + 1];
  __shared__ int hit[NDT_SCORE_TILE][LOC_PTS + 1];
  const int n = min(cap, max(*n_dev, 0));
  const int base = blockIdx.x * LOC_PTS;
  if (base >= n) return;                     // as k_ndt_assoc: rows past the last element are never written, never read
  const int p0 = blockIdx.y * NDT_SCORE_TILE;
  const int tile = min(NDT_SCORE_TILE, n_pose - p0);
  if (tile <= 0) return;
  for (int t = threadIdx.x; t < tile * 12; t += 256) pose[t / 12][t % 12] = T[(size_t)(p0 + t / 12) * 16 + t % 12];
  const int k = threadIdx.x / NDT_LANES, sub = threadIdx.x % NDT_LANES;
  const int i = base + k;
  double el[Scan::ELEM];
#pragma unroll
  for (int j = 0; j < Scan::ELEM; ++j) el[j] = 0.0;
  if (i < n) {
#pragma unroll
    for (int j = 0; j < Scan::ELEM; ++j) el[j] = elems[(size_t)i * Scan::ELEM + j];
  }
  const bool live = i < n && Scan::valid(el);
  __syncthreads();
  for (int j = 0; j < tile; ++j) {
    double v = 0.0;
    int ok = 0;
    if (live) {
      double q[3], e, w, y[3], B[6];
      if (Scan::hit(m, gs, pose[j], el, sub, neighbours, q, e, w, y, B)) {
        v = loc_mul(gs.nd1, e);
        ok = 1;
      }
    }
    // the element's cells in lookup order (every lane of the wave takes part in the shuffles)
    double term = 0.0;
    int any = 0;
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      const double vc = __shfl(v, c, NDT_LANES);
      const int okc = __shfl(ok, c, NDT_LANES);
      if (okc) term = loc_add(term, vc), any = 1;
    }
    if (sub == 0) sc[j][k] = term, hit[j][k] = any;
  }
  __syncthreads();
  if ((int)threadIdx.x < tile) {
    const int j = threadIdx.x;
    double s = 0.0, cnt = 0.0;
    for (int p = 0; p < LOC_PTS; ++p) s = loc_add(s, sc[j][p]), cnt = loc_add(cnt, hit[j][p] ? 1.0 : 0.0);
    double *o = partial + ((size_t)(p0 + j) * gridDim.x + blockIdx.x) * 2;
    o[0] = s, o[1] = cnt;
  }
}
using NdtScoreKernel = decltype(&k_ndt_score<NdtPoints>);

// Thread (pose, sg, col) adds the rows of run sg of the pose's blocks in order, thread (pose, 0, col) the LOC_SEG runs
// in order: loc_sum_rows restated for two columns, NDT_REDUCE_POSES poses per workgroup.  nb = the partial rows of one
// pose; as in launch B only the rows that hold points are read.
__global__ __launch_bounds__(256) void k_ndt_score_reduce(const double *__restrict__ partial, int nb, const int *__restrict__ n_dev,
                                                           int cap, int n_pose, double *__restrict__ score) {
  __shared__ double seg[NDT_REDUCE_POSES][LOC_SEG][2];
  const int n = min(cap, max(*n_dev, 0));
  const int rows = min(nb, (n + LOC_PTS - 1) / LOC_PTS);
  const int lp = threadIdx.x / (LOC_SEG * 2), sg = (threadIdx.x / 2) % LOC_SEG, col = threadIdx.x % 2;
  const int p = blockIdx.x * NDT_REDUCE_POSES + lp;
  if (p < n_pose) {
    const int per = (rows + LOC_SEG - 1) / LOC_SEG;
    const int b1 = min(rows, (sg + 1) * per);
    const double *src = partial + (size_t)p * nb * 2 + col;
    double s = 0.0;
    for (int b = sg * per; b < b1; ++b) s = loc_add(s, src[(size_t)b * 2]);
    seg[lp][sg][col] = s;
  }
  __syncthreads();
  if (p < n_pose && sg == 0) {
    double s = 0.0;
    for (int i = 0; i < LOC_SEG; ++i) s = loc_add(s, seg[lp][i][col]);
    score[(size_t)p * 2 + col] = s;
  }
}

// true where pose (s, i) comes before pose (bs, bi) in the order (score descending, index ascending); bi < 0: no pose yet
__device__ inline bool ndt_top_before(double s, int i, double bs, int bi) { return bi < 0 || s > bs || (s == bs && i < bi); }

// One workgroup.  A pose qualifies with count >= min_corr and a score that is not NaN.  Round r takes the first pose, in
// the order (score descending, index ascending), that comes after the pose of round r - 1: a scan by every thread over
// its poses, then a reduction whose result does not depend on the order of arrival.  Slots past the last qualifying
// pose get index -1 and the pose of slot 0 (T[0] where nobody qualifies).
__global__ __launch_bounds__(NDT_TOP_THREADS) void k_ndt_top(const double *__restrict__ score, const double *__restrict__ T,
                                                              int n_pose, int min_corr, int k, int *__restrict__ top_index,
                                                              double *__restrict__ T_top, int *__restrict__ n_top) {
  __shared__ double ws[NDT_TOP_THREADS / 64];
  __shared__ int wi[NDT_TOP_THREADS / 64];
  __shared__ double pick_s;
  __shared__ int pick_i;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  k = min(k, SPS_NDT_MAX_HYP);
  double ps = INFINITY;    // the previous pick; (inf, -1) comes before every pose
  int pi = -1, filled = 0, first = 0;
  for (int r = 0; r < k; ++r) {
    double bs = 0.0;
    int bi = -1;
    for (int p = t; p < n_pose; p += NDT_TOP_THREADS) {
      const double s = score[(size_t)p * 2], c = score[(size_t)p * 2 + 1];
      if (!(c >= (double)min_corr) || s != s) continue;
      if (!(s < ps || (s == ps && p > pi))) continue;       // taken in an earlier round
      if (ndt_top_before(s, p, bs, bi)) bs = s, bi = p;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(bs, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi >= 0 && ndt_top_before(os, oi, bs, bi)) bs = os, bi = oi;
    }
    if (lane == 0) ws[wave] = bs, wi[wave] = bi;
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < NDT_TOP_THREADS / 64; ++w)
        if (wi[w] >= 0 && ndt_top_before(ws[w], wi[w], bs, bi)) bs = ws[w], bi = wi[w];
      pick_s = bs, pick_i = bi;
    }
    __syncthreads();
    ps = pick_s, pi = pick_i;
    __syncthreads();                                        // the next round writes ws, wi and the pick again
    if (pi < 0) break;                                      // the same for every thread
    if (r == 0) first = pi;
    if (t == 0) top_index[r] = pi;
    if (t < 16) T_top[(size_t)r * 16 + t] = T[(size_t)pi * 16 + t];
    filled = r + 1;
  }
  for (int r = filled; r < k; ++r) {
    if (t == 0) top_index[r] = -1;
    if (t < 16) T_top[(size_t)r * 16 + t] = T[(size_t)first * 16 + t];
  }
  if (t == 0) *n_top = filled;
}

#pragma clang fp contract(fast)
