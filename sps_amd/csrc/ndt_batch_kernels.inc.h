// ndt_batch_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after ndt_kernels.inc.h): the
// NDT localiser from several start poses at once, with best-score selection (host side: ndt_batch_host.inc.h; ABI: the
// "NDT localiser, several hypotheses" section of include/sps_hip.h).
//
//   k_loc_init_batch    T_out[k] = T_init[k], status[k] = (1, 0, 0, 0), done[k] = 0
//   k_ndt_assoc_batch   (launch A)  grid (blocks, K): ndt_assoc_body of hypothesis blockIdx.y (a template over the scan, as
//                       k_ndt_assoc)
//   k_loc_solve_batch   (launch B)  grid K: loc_solve_body of hypothesis blockIdx.x
//   k_ndt_select        the score and the count of every hypothesis at its final pose, and the best of them
//
// The scan (points or, NdtCells, source cells) and the map are read by all hypotheses; a hypothesis owns its pose, its
// done flag, its partial rows (partial[k][block][LOC_TERMS]), its status, trace and normal rows.  Per hypothesis every
// operation and the order of every sum are those of k_ndt_assoc / k_loc_solve, whose bodies these kernels call, so
// hypothesis k of a batch has the bits of a single alignment from T_init[k].  Stores are plain vector stores; nothing here
// is atomic.

#pragma clang fp contract(off)

constexpr int NDT_SELECT_GROUPS = 4;   // hypotheses k_ndt_select sums at a time (256 threads each)

__global__ __launch_bounds__(64) void k_loc_init_batch(const double *__restrict__ T_init, int n_hyp, double *__restrict__ T_out,
                                                       int *__restrict__ status, int *__restrict__ done) {
  const int k = blockIdx.x, t = threadIdx.x;
  if (k >= n_hyp) return;
  if (t < 16) T_out[(size_t)k * 16 + t] = T_init[(size_t)k * 16 + t];
  if (t < 4) status[k * 4 + t] = t == 0 ? 1 : 0;
  if (t == 0) done[k] = 0;
}

// Launch A.  nb = the partial rows of one hypothesis (gridDim.x); all = 1: the pass after the last iteration, which
// evaluates every hypothesis at its final pose whatever its done flag says.
template <class Scan>
__global__ __launch_bounds__(256) void k_ndt_assoc_batch(const double *__restrict__ elems, const int *__restrict__ n_dev, int cap,
                                                          NdtMap m, NdtGauss gs, int neighbours, int n_hyp,
                                                          const double *__restrict__ T, const int *__restrict__ done, int all,
                                                          double *__restrict__ partial) {
  __shared__ NdtAssocLds lds;
  const int k = blockIdx.y;
  if (k >= n_hyp) return;
  if (!all && done[k]) return;
  ndt_assoc_body<Scan>(elems, n_dev, cap, m, gs, neighbours, T + (size_t)k * 16, partial + (size_t)k * gridDim.x * LOC_TERMS, lds);
}
using NdtAssocBatchKernel = decltype(&k_ndt_assoc_batch<NdtPoints>);

// Launch B, one workgroup of 256 per hypothesis.  nb = the partial rows of one hypothesis.
__global__ __launch_bounds__(256) void k_loc_solve_batch(const double *__restrict__ partial, int nb, const int *__restrict__ n_dev,
                                                          int cap, int iter, int iters, int min_corr, double tol_t, double tol_r,
                                                          int n_hyp, const double *__restrict__ T_init, double *__restrict__ T,
                                                          int *__restrict__ status, int *__restrict__ done,
                                                          double *__restrict__ trace, double *__restrict__ normal) {
  __shared__ double seg[LOC_SEG][32];
  __shared__ double tot[32];
  const int k = blockIdx.x;
  if (k >= n_hyp) return;
  loc_solve_body(partial + (size_t)k * nb * LOC_TERMS, n_dev, cap, iter, min_corr, tol_t, tol_r, T_init + (size_t)k * 16,
                 T + (size_t)k * 16, status + k * 4, done + k, trace + (size_t)k * iters * 4,
                 normal ? normal + (size_t)k * iters * 28 : nullptr, seg, tot);
}

// One workgroup of 256 * NDT_SELECT_GROUPS, after the pass of k_ndt_assoc_batch with all = 1.  Group g adds the rows of
// hypotheses g, g + NDT_SELECT_GROUPS, ... as loc_sum_rows does for launch B; final[k] = (score, points counted).  Thread 0
// then takes the highest score among the hypotheses with status 0 or 1 and at least min_corr points counted; a tie stays
// with the lowest k.  best = (k, its status, its count, n_hyp) and T_best = T[k]; nobody qualifies: (-1, -1, 0, n_hyp) and
// T_best = T_init[0].
__global__ __launch_bounds__(256 * NDT_SELECT_GROUPS) void k_ndt_select(const double *__restrict__ partial, int nb,
                                                                         const int *__restrict__ n_dev, int cap, int n_hyp,
                                                                         int min_corr, const int *__restrict__ status,
                                                                         const double *__restrict__ T,
                                                                         const double *__restrict__ T_init,
                                                                         double *__restrict__ final, int *__restrict__ best,
                                                                         double *__restrict__ T_best) {
  __shared__ double seg[NDT_SELECT_GROUPS][LOC_SEG][32];
  __shared__ double tot[NDT_SELECT_GROUPS][32];
  __shared__ double score[SPS_NDT_MAX_HYP];
  __shared__ int count[SPS_NDT_MAX_HYP];
  const int n = min(cap, max(*n_dev, 0));
  const int rows = min(nb, (n + LOC_PTS - 1) / LOC_PTS);
  const int g = threadIdx.x >> 8, t = threadIdx.x & 255;
  n_hyp = min(n_hyp, SPS_NDT_MAX_HYP);
  for (int k0 = 0; k0 < n_hyp; k0 += NDT_SELECT_GROUPS) {
    const int k = k0 + g;
    // a group past the last hypothesis adds no rows but keeps the workgroup's barriers
    loc_sum_rows(partial + (size_t)min(k, n_hyp - 1) * nb * LOC_TERMS, k < n_hyp ? rows : 0, t, seg[g], tot[g]);
    if (t == 0 && k < n_hyp) {
      score[k] = tot[g][27], count[k] = (int)tot[g][28];
      final[2 * k] = tot[g][27], final[2 * k + 1] = tot[g][28];
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int b = -1;
  double top = -INFINITY;
  for (int k = 0; k < n_hyp; ++k) {
    const int code = status[k * 4];
    if ((code == 0 || code == 1) && count[k] >= min_corr && score[k] > top) b = k, top = score[k];   // NaN never wins
  }
  best[0] = b, best[1] = b >= 0 ? status[b * 4] : -1, best[2] = b >= 0 ? count[b] : 0, best[3] = n_hyp;
  const double *src = b >= 0 ? T + (size_t)b * 16 : T_init;
  for (int i = 0; i < 16; ++i) T_best[i] = src[i];
}

#pragma clang fp contract(fast)
