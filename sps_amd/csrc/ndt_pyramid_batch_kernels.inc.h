// ndt_pyramid_batch_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after
// ndt_d2d_kernels.inc.h): the coarse-to-fine NDT alignment from several start poses at once (host side:
// ndt_pyramid_batch_host.inc.h; ABI: the "NDT localiser, pyramid, several hypotheses" section of include/sps_hip.h).
//
//   k_ndt_pyr_init_batch    grid (blocks, K): T_out[k] = T_init[k], status[k] = (1, 0, 0, 0), the state words of k 0,
//                           level[k][s] = -1, the trace and normal rows of k 0
//   k_ndt_pyr_assoc_batch   (launch A of a slot)  grid (blocks, K): ndt_assoc_body of hypothesis blockIdx.y against the map of
//                           the level its state names
//   k_ndt_pyr_solve_batch   (launch B of a slot)  grid K: loc_sum_rows + loc_solve_step + ndt_pyr_handoff of hypothesis
//                           blockIdx.x
//   k_ndt_pyr_final_batch   (after the last slot)  grid (blocks, K): ndt_assoc_body of every hypothesis against the scoring
//                           level, which it finds on the device
// The three are templates over the scan (NdtPoints: sps_ndt_pyramid_align_batch; NdtCells, a slice of source cells per
// level: sps_ndt_pyramid_align_d2d_batch).
//
// The scan points and the levels are read by all hypotheses; a hypothesis owns its pose, its NDT_PYR_STATE state words
// (done, level, slots used per level), its partial rows (partial[k][block][LOC_TERMS], the layout of
// ndt_batch_kernels.inc.h), its status, trace, normal and level rows.  Hypotheses stand at different levels in the same
// slot; one whose state says done sits out.  Per hypothesis every operation and the order of every sum are those of
// k_ndt_pyr_assoc / k_ndt_pyr_solve, whose bodies and whose handoff rule these kernels call, so hypothesis k has the bits
// of sps_ndt_pyramid_align (sps_ndt_pyramid_align_d2d) from T_init[k].  The selection is k_ndt_select of
// ndt_batch_kernels.inc.h, given the count of the scoring level.  Stores are plain vector stores; nothing here is atomic.

#pragma clang fp contract(off)

// Block (0, k) sets the pose, the status and the state of hypothesis k; all blocks of row k clear its per-slot rows
// (normal may be null; iters = 0 leaves trace and level untouched).
__global__ __launch_bounds__(256) void k_ndt_pyr_init_batch(const double *__restrict__ T_init, int n_hyp, int iters,
                                                             double *__restrict__ T_out, int *__restrict__ status,
                                                             int *__restrict__ state, double *__restrict__ trace,
                                                             double *__restrict__ normal, int *__restrict__ level) {
  const int k = blockIdx.y, t = threadIdx.x;
  if (k >= n_hyp) return;
  if (blockIdx.x == 0) {
    if (t < 16) T_out[(size_t)k * 16 + t] = T_init[(size_t)k * 16 + t];
    if (t < 4) status[k * 4 + t] = t == 0 ? 1 : 0;  // 1 = slots exhausted, unless a slot says otherwise
    if (t < NDT_PYR_STATE) state[k * NDT_PYR_STATE + t] = 0;
  }
  const int stride = gridDim.x * 256;
  const size_t row = (size_t)k * iters;
  for (int i = blockIdx.x * 256 + t; i < iters * 28; i += stride) {
    if (i < iters) level[row + i] = -1;
    if (i < iters * 4) trace[row * 4 + i] = 0.0;
    if (normal) normal[row * 28 + i] = 0.0;
  }
}

// Launch A.  Grid (the workgroups of k_ndt_pyr_assoc, K).  The level is the same for every thread of a workgroup: it goes
// through a scalar register, and the level's descriptor is read from the device array, as in k_ndt_pyr_assoc.  The elements
// and their count are the level's (Scan::level_elems, Scan::level_count: the same points at every level, a slice of source
// cells per level).
template <class Scan>
__global__ __launch_bounds__(256) void k_ndt_pyr_assoc_batch(const double *__restrict__ elems, const int *__restrict__ n_dev,
                                                              int cap, const NdtPyrLevel *__restrict__ levels, int n_levels,
                                                              int neighbours, int n_hyp, const double *__restrict__ T,
                                                              const int *__restrict__ state, double *__restrict__ partial) {
  __shared__ NdtAssocLds lds;
  const int k = blockIdx.y;
  if (k >= n_hyp) return;
  const int *st = state + k * NDT_PYR_STATE;
  if (st[0]) return;
  const int l = __builtin_amdgcn_readfirstlane(min(max(st[1], 0), n_levels - 1));
  const NdtPyrLevel d = levels[l];
  ndt_assoc_body<Scan>(Scan::level_elems(elems, cap, l), Scan::level_count(n_dev, l), cap, d.m, d.gs, neighbours,
                       T + (size_t)k * 16, partial + (size_t)k * gridDim.x * LOC_TERMS, lds);
}
using NdtPyrAssocBatchKernel = decltype(&k_ndt_pyr_assoc_batch<NdtPoints>);

// Launch B, one workgroup of 256 per hypothesis.  nb = the partial rows of one hypothesis; the rows summed are those of the
// level's count.  T_init is read from the device (only when the status becomes 2 or 3), as in k_loc_solve_batch.
template <class Scan>
__global__ __launch_bounds__(256) void k_ndt_pyr_solve_batch(const double *__restrict__ partial, int nb,
                                                              const int *__restrict__ n_dev, int cap, int slot, int iters,
                                                              int n_levels, NdtPyrCaps caps, int min_corr, double tol_t,
                                                              double tol_r, int n_hyp, const double *__restrict__ T_init,
                                                              double *__restrict__ T, int *__restrict__ status,
                                                              int *__restrict__ state, double *__restrict__ trace,
                                                              double *__restrict__ normal, int *__restrict__ level) {
  __shared__ double seg[LOC_SEG][32];
  __shared__ double tot[32];
  __shared__ LocSolveWork work;   // thread 0's alone: in workgroup memory, so that the kernel uses no scratch memory
  const int k = blockIdx.x;
  if (k >= n_hyp) return;
  state += k * NDT_PYR_STATE;
  if (state[0]) return;
  status += k * 4;
  // every thread reads the level here, before the barriers of loc_sum_rows: thread 0 rewrites state[1] in the handoff below
  const int l = min(max(state[1], 0), n_levels - 1);
  const int n = min(cap, max(*Scan::level_count(n_dev, l), 0));
  loc_sum_rows(partial + (size_t)k * nb * LOC_TERMS, (n + LOC_PTS - 1) / LOC_PTS, threadIdx.x, seg, tot);
  if (threadIdx.x != 0) return;
  level[(size_t)k * iters + slot] = l;
  status[3] = l;
  double vn, th;
  if (loc_solve_step_in(work, tot, slot, min_corr, T_init + (size_t)k * 16, T + (size_t)k * 16, status,
                        trace + (size_t)k * iters * 4, normal ? normal + (size_t)k * iters * 28 : nullptr, vn, th) >= 0) {
    state[0] = 1;
    return;
  }
  ndt_pyr_handoff(l, Scan::next(n_dev, cap, l, n_levels, min_corr), caps, vn < tol_t && th < tol_r, status, state);
}
using NdtPyrSolveBatchKernel = decltype(&k_ndt_pyr_solve_batch<NdtPoints>);

// The pass after the last slot.  Grid of launch A.  Every hypothesis, whatever its state says, once more at its final pose
// against the scoring level: the last level of the chain every hypothesis walks (Scan::last: the finest for points, the last
// level that source cells do not skip), found on the device and kept in a scalar register.  Block (0, 0) leaves that level's
// count and the level in the two spare state words of hypothesis 0 (NDT_PYR_FINAL_COUNT, NDT_PYR_FINAL_LEVEL), which no
// launch reads before k_ndt_select clips its rows by the first of them.
constexpr int NDT_PYR_FINAL_COUNT = 6, NDT_PYR_FINAL_LEVEL = 7;
static_assert(NDT_PYR_FINAL_LEVEL < NDT_PYR_STATE && 2 + NDT_PYR_MAX <= NDT_PYR_FINAL_COUNT, "the spare state words");

template <class Scan>
__global__ __launch_bounds__(256) void k_ndt_pyr_final_batch(const double *__restrict__ elems, const int *__restrict__ n_dev,
                                                              int cap, const NdtPyrLevel *__restrict__ levels, int n_levels,
                                                              int neighbours, int min_corr, int n_hyp,
                                                              const double *__restrict__ T, int *__restrict__ state,
                                                              double *__restrict__ partial) {
  __shared__ NdtAssocLds lds;
  const int k = blockIdx.y;
  if (k >= n_hyp) return;
  const int l = __builtin_amdgcn_readfirstlane(min(max(Scan::last(n_dev, cap, n_levels, min_corr), 0), n_levels - 1));
  const int *count = Scan::level_count(n_dev, l);
  if (blockIdx.x == 0 && k == 0 && threadIdx.x == 0) {
    state[NDT_PYR_FINAL_COUNT] = *count;
    state[NDT_PYR_FINAL_LEVEL] = l;
  }
  const NdtPyrLevel d = levels[l];
  ndt_assoc_body<Scan>(Scan::level_elems(elems, cap, l), count, cap, d.m, d.gs, neighbours, T + (size_t)k * 16,
                       partial + (size_t)k * gridDim.x * LOC_TERMS, lds);
}
using NdtPyrFinalBatchKernel = decltype(&k_ndt_pyr_final_batch<NdtPoints>);

#pragma clang fp contract(fast)
