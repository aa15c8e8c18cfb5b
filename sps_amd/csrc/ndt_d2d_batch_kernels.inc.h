// ndt_d2d_batch_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after ndt_d2d_kernels.inc.h,
// which follows ndt_batch_kernels.inc.h and ndt_search_kernels.inc.h): distribution-to-distribution NDT from several start
// poses at once, and the D2D score of many poses (host side: ndt_d2d_batch_host.inc.h; ABI: the "NDT localiser,
// distribution to distribution, several poses" section of include/sps_hip.h).
//
//   k_ndt_d2d_assoc_batch   (launch A)  grid (blocks, K): ndt_d2d_assoc_body of hypothesis blockIdx.y
//   k_ndt_d2d_score         grid (source blocks, pose tiles): partial[pose][block] = (score, sources counted) of the
//                           block's LOC_PTS source records at every pose of the tile
//
// The initialisation, launch B and the select are k_loc_init_batch, k_loc_solve_batch and k_ndt_select unchanged, the
// second launch of the scorer is k_ndt_score_reduce unchanged: all of them take their row count from the count they are
// handed, which here is the source count.  Per hypothesis every operation and the order of every sum are those of
// k_ndt_d2d_assoc / k_loc_solve, so hypothesis k of a batch has the bits of sps_ndt_align_d2d from T_init[k]; per source and
// pose k_ndt_d2d_score calls what phase 1 of ndt_d2d_assoc_body calls (loc_transform, ndt_rotate_cov, ndt_cell_of,
// ndt_d2d_hit) and forms of the 29 terms only the score (27) and the count (28), in the orders of ndt_assoc_reduce and
// loc_sum_rows, so score[pose] has the bits of final_dev[k] of sps_ndt_align_d2d_batch(iters = 0) started at that pose.
// Everything is float64, every operation is rounded on its own, stores are plain vector stores, nothing is atomic.

#pragma clang fp contract(off)

// Launch A.  nb = the partial rows of one hypothesis (gridDim.x); all = 1: the pass after the last iteration, which
// evaluates every hypothesis at its final pose whatever its done flag says.
__global__ __launch_bounds__(256) void k_ndt_d2d_assoc_batch(const double *__restrict__ src, const int *__restrict__ n_src, int cap,
                                                              NdtMap m, NdtGauss gs, int neighbours, int n_hyp,
                                                              const double *__restrict__ T, const int *__restrict__ done,
                                                              int all, double *__restrict__ partial) {
  __shared__ NdtAssocLds lds;
  const int k = blockIdx.y;
  if (k >= n_hyp) return;
  if (!all && done[k]) return;
  ndt_d2d_assoc_body(src, n_src, cap, m, gs, neighbours, T + (size_t)k * 16, partial + (size_t)k * gridDim.x * LOC_TERMS, lds);
}

// NDT_LANES lanes per source record, LOC_PTS records per workgroup, as in k_ndt_d2d_assoc; the poses of a tile, the LDS and
// the last step are those of k_ndt_score.  The workgroup reads its records once and walks the poses of its tile: every lane
// of a valid source forms q and Cw at the pose (the same values on its eight lanes, as in the body), lane c < neighbours
// looks up cell c of q, the source's lane 0 adds the contributing cells in lookup order; then thread j adds the LOC_PTS
// sources of pose j in index order.  A source that is not valid, or lies beyond the cells built, adds 0 and is not counted,
// which is what its row of zero terms adds in the body.  nb = gridDim.x = the partial rows of one pose.
__global__ __launch_bounds__(256) void k_ndt_d2d_score(const double *__restrict__ src, const int *__restrict__ n_src, int cap,
                                                        NdtMap m, NdtGauss gs, int neighbours, const double *__restrict__ T,
                                                        int n_pose, double *__restrict__ partial) {
  __shared__ double pose[NDT_SCORE_TILE][12];
  __shared__ double sc[NDT_SCORE_TILE][LOC_PTS + 1];
  __shared__ int hit[NDT_SCORE_TILE][LOC_PTS + 1];
  const int n = min(cap, max(*n_src, 0));
  const int base = blockIdx.x * LOC_PTS;
  if (base >= n) return;                     // as k_ndt_d2d_assoc: rows past the last source are never written, never read
  const int p0 = blockIdx.y * NDT_SCORE_TILE;
  const int tile = min(NDT_SCORE_TILE, n_pose - p0);
  if (tile <= 0) return;
  for (int t = threadIdx.x; t < tile * 12; t += 256) pose[t / 12][t % 12] = T[(size_t)(p0 + t / 12) * 16 + t % 12];
  const int k = threadIdx.x / NDT_LANES, sub = threadIdx.x % NDT_LANES;
  const int i = base + k;
  double s[NDT_SRC_REC];
#pragma unroll
  for (int j = 0; j < NDT_SRC_REC; ++j) s[j] = 0.0;
  if (i < n) {
#pragma unroll
    for (int j = 0; j < NDT_SRC_REC; ++j) s[j] = src[(size_t)i * NDT_SRC_REC + j];
  }
  const bool live = i < n && s[9] != 0.0;
  __syncthreads();
  for (int j = 0; j < tile; ++j) {
    double v = 0.0;
    int ok = 0;
    if (live) {
      double q[3], Cw[6];
      loc_transform(pose[j], s[0], s[1], s[2], q);
      ndt_rotate_cov(pose[j], s + 3, Cw);
      const int cell = sub < neighbours ? ndt_cell_of(m, q, sub) : -1;
      double e, w, y[3], B[6];
      if (cell >= 0 && ndt_d2d_hit(q, Cw, m.rec + (size_t)cell * NDT_REC, gs, e, w, y, B)) {
        v = loc_mul(gs.nd1, e);
        ok = 1;
      }
    }
    // the source's cells in lookup order (every lane of the wave takes part in the shuffles)
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
    double t = 0.0, cnt = 0.0;
    for (int p = 0; p < LOC_PTS; ++p) t = loc_add(t, sc[j][p]), cnt = loc_add(cnt, hit[j][p] ? 1.0 : 0.0);
    double *o = partial + ((size_t)(p0 + j) * gridDim.x + blockIdx.x) * 2;
    o[0] = t, o[1] = cnt;
  }
}

#pragma clang fp contract(fast)
