// ndt_pyramid_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after ndt_update_kernels.inc.h):
// the NDT localiser registering coarse to fine over a pyramid of cell maps, static or (ndt_online_kernels.inc.h)
// dynamic (host side: ndt_pyramid_host.inc.h; ABI: the "NDT localiser, multi-resolution pyramid" section of include/sps_hip.h).
//
//   k_ndt_pyr_init    T_out = T_init, status = (1, 0, 0, 0), the state words 0, level[s] = -1, trace and normal rows 0
//   k_ndt_pyr_assoc   (launch A of a slot)  ndt_assoc_body on the scan's elements of the level the state names, against
//                     that level's map
//   k_ndt_pyr_solve   (launch B of a slot)  loc_sum_rows + loc_solve_step, then the handoff rule (ndt_pyr_handoff: its one
//                     definition, shared with k_ndt_pyr_solve_batch of ndt_pyramid_batch_kernels.inc.h)
// Both are templates over the scan (NdtPoints of ndt_kernels.inc.h: the same points at every level, level l + 1 follows l;
// NdtCells of ndt_d2d_kernels.inc.h: a slice of source cells per level, levels with too few valid cells are skipped).
//
// The levels are the maps k_radius_cells_insert and k_ndt_cells build, one NdtPyrLevel (map + Gaussian fit) each in a device
// array.  Which level a slot runs at is decided on the device: the state words live in the caller's scratch behind the
// partial rows, launch B of a slot writes them and both launches of the next slot read them, so the host issues the same
// launches whatever happens.  Per slot every operation and the order of every sum are those of k_ndt_assoc / k_loc_solve,
// whose bodies these kernels call: a pyramid of one level has the bits of sps_ndt_align, and one of several levels those of
// as many sps_ndt_align calls chained through their end poses.  Stores are plain vector stores; nothing here is atomic.

#pragma clang fp contract(off)

constexpr int NDT_PYR_MAX = 4;        // SPS_NDT_PYR_MAX_LEVELS
constexpr int NDT_PYR_STATE = 8;      // ints of state: done, level, slots used at each level, two spare
static_assert(NDT_PYR_MAX == SPS_NDT_PYR_MAX_LEVELS, "include/sps_hip.h states the level limit");

struct NdtPyrLevel {
  NdtMap m;
  NdtGauss gs;
};

struct NdtPyrCaps {
  int v[NDT_PYR_MAX];      // level_iters: the most slots a level may use
};

// A pyramid of a context: the levels on the host, for the getters and the by-value kernels, and their device copy; a
// dynamic pyramid also has every level's NdtDyn, in a device array beside the levels'.  A context has two (sps_ctx): the
// single map of sps_ndt_map_build[_dynamic], one level whose gs is not set, and that of sps_ndt_pyramid_build[_dynamic].
struct NdtPyramid {
  int n_levels = 0;        // 0: none built
  std::vector<void *> allocs;         // the device memory of the levels and of the two arrays below, owned
  NdtPyrLevel lv[NDT_PYR_MAX]{};
  const NdtPyrLevel *dev = nullptr;   // [NDT_PYR_MAX]
  bool dynamic = false;    // built by a *_build_dynamic
  NdtDyn dyn[NDT_PYR_MAX]{};
  const NdtDyn *dyn_dev = nullptr;    // [NDT_PYR_MAX], dynamic only
};

// Block 0 sets the pose, the status and the state; all blocks clear the per-slot rows (normal and level may be null / empty).
__global__ __launch_bounds__(256) void k_ndt_pyr_init(LocPose T, int iters, double *__restrict__ T_out, int *__restrict__ status,
                                                       int *__restrict__ state, double *__restrict__ trace,
                                                       double *__restrict__ normal, int *__restrict__ level) {
  const int t = threadIdx.x;
  if (blockIdx.x == 0) {
    if (t < 16) T_out[t] = T.m[t];
    if (t < 4) status[t] = t == 0 ? 1 : 0;  // 1 = slots exhausted, unless a slot says otherwise
    if (t < NDT_PYR_STATE) state[t] = 0;
  }
  const int stride = gridDim.x * 256;
  for (int i = blockIdx.x * 256 + t; i < iters * 28; i += stride) {
    if (i < iters) level[i] = -1;
    if (i < iters * 4) trace[i] = 0.0;
    if (normal) normal[i] = 0.0;
  }
}

// Launch A.  Grid and workgroup of k_ndt_assoc.  The level is the same for every thread of the grid: it goes through a
// scalar register, and the level's descriptor is read from the device array (a by-value array indexed by it would live in
// scratch).
template <class Scan>
__global__ __launch_bounds__(256) void k_ndt_pyr_assoc(const double *__restrict__ elems, const int *__restrict__ n_dev, int cap,
                                                        const NdtPyrLevel *__restrict__ levels, int n_levels, int neighbours,
                                                        const double *__restrict__ T, const int *__restrict__ state,
                                                        double *__restrict__ partial) {
  __shared__ NdtAssocLds lds;
  if (state[0]) return;
  const int l = __builtin_amdgcn_readfirstlane(min(max(state[1], 0), n_levels - 1));
  const NdtPyrLevel d = levels[l];
  ndt_assoc_body<Scan>(Scan::level_elems(elems, cap, l), Scan::level_count(n_dev, l), cap, d.m, d.gs, neighbours, T, partial,
                       lds);
}
using NdtPyrAssocKernel = decltype(&k_ndt_pyr_assoc<NdtPoints>);

// The handoff rule, by the one thread that made a step at level l (ndt_pyr_solve_body below; k_ndt_pyr_solve_batch in
// ndt_pyramid_batch_kernels.inc.h runs it once per hypothesis): that level's count of used slots goes up; a converged step
// ends the call with status 0 on the last level and hands the pose to level `next` otherwise; a step that is not converged
// does the same once the level has used its cap, except that the status stays 1.  next: the level that follows l, < 0
// where l is the last (the scan's `next`: l + 1 for points, while source cells skip levels).  state: the call's (the
// hypothesis') words.
__device__ inline void ndt_pyr_handoff(int l, int next, NdtPyrCaps caps, bool converged, int *__restrict__ status,
                                       int *__restrict__ state) {
  const int used = state[2 + l] + 1;
  state[2 + l] = used;
  const int cap_l = l == 0 ? caps.v[0] : (l == 1 ? caps.v[1] : (l == 2 ? caps.v[2] : caps.v[3]));
  const bool last = next < 0;
  if (converged) {
    if (last) {
      status[0] = 0;
      state[0] = 1;
    } else {
      state[1] = next;
    }
  } else if (used >= cap_l) {
    if (last)
      state[0] = 1;
    else
      state[1] = next;
  }
}

// The step of launch B, by a workgroup of 256 whose call is live: the n rows' partial sums (loc_sum_rows), then thread 0
// alone: loc_solve_step at level l and the handoff to `next`.
__device__ inline void ndt_pyr_solve_body(const double *__restrict__ partial, int n, int slot, int l, int next, NdtPyrCaps caps,
                                          int min_corr, double tol_t, double tol_r, const LocPose &T_init, double *__restrict__ T,
                                          int *__restrict__ status, int *__restrict__ state, double *__restrict__ trace,
                                          double *__restrict__ normal, int *__restrict__ level, double (*seg)[32], double *tot) {
  loc_sum_rows(partial, (n + LOC_PTS - 1) / LOC_PTS, threadIdx.x, seg, tot);
  if (threadIdx.x != 0) return;
  level[slot] = l;
  status[3] = l;
  double vn, th;
  if (loc_solve_step(tot, slot, min_corr, T_init.m, T, status, trace, normal, vn, th) >= 0) {
    state[0] = 1;
    return;
  }
  ndt_pyr_handoff(l, next, caps, vn < tol_t && th < tol_r, status, state);
}

// Launch B, one workgroup of 256.  After a step at level l that level's count of used slots goes up; a converged step
// (|v| < tol_t and |omega| < tol_r) ends the call with status 0 on the last level and hands the pose to level l + 1
// otherwise; a step that is not converged does the same once the level has used its cap, except that the status stays 1.
// Status 2 and 3 are final at any level.  status = (code, slots used, count of the last live slot, its level).  The rows are
// those of the level's elements (Scan::level_count), the level that follows is the scan's (Scan::next).
template <class Scan>
__global__ __launch_bounds__(256) void k_ndt_pyr_solve(const double *__restrict__ partial, const int *__restrict__ n_dev, int cap,
                                                        int slot, int n_levels, NdtPyrCaps caps, int min_corr, double tol_t,
                                                        double tol_r, LocPose T_init, double *__restrict__ T,
                                                        int *__restrict__ status, int *__restrict__ state,
                                                        double *__restrict__ trace, double *__restrict__ normal,
                                                        int *__restrict__ level) {
  __shared__ double seg[LOC_SEG][32];
  __shared__ double tot[32];
  if (state[0]) return;
  const int l = min(max(state[1], 0), n_levels - 1);
  const int n = min(cap, max(*Scan::level_count(n_dev, l), 0));
  ndt_pyr_solve_body(partial, n, slot, l, Scan::next(n_dev, cap, l, n_levels, min_corr), caps, min_corr, tol_t, tol_r, T_init, T,
                     status, state, trace, normal, level, seg, tot);
}
using NdtPyrSolveKernel = decltype(&k_ndt_pyr_solve<NdtPoints>);

#pragma clang fp contract(fast)
