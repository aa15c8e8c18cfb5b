// ndt_d2d_pyramid_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after
// ndt_online_kernels.inc.h): distribution-to-distribution NDT registered coarse to fine (host side:
// ndt_d2d_pyramid_host.inc.h; ABI: the "NDT localiser, distribution to distribution, pyramid" section of include/sps_hip.h;
// DESIGN.md 8p).  The scan's cells are built once per level, each level at a resolution of its own, and registered against
// the pyramid of map cells of ndt_pyramid_kernels.inc.h, the pose handed from level to level on the device.
//
//   k_ndt_pyr_src_lookup .. k_ndt_pyr_src_records   the seven launches of the source build, grid (blocks of one level, levels)
//   k_ndt_d2d_pyr_assoc    (launch A of a slot)  ndt_d2d_assoc_body on the source slice and the map of the level the state names
//   k_ndt_d2d_pyr_solve    (launch B of a slot)  ndt_pyr_solve_body with the rows of that level's sources, and a handoff that
//                          skips the levels whose valid sources are fewer than min_corr
//
// Nothing is computed here.  The source kernels pick their level, blockIdx.y, and call the bodies of
// ndt_update_kernels.inc.h and ndt_src_records_body with that level's slice of the scratch, as ndt_online_kernels.inc.h does
// for the online pyramid: level l gets the bits of k_ndt_src_* at that level's resolution and min_points.  The two launches
// of a slot call the bodies of k_ndt_d2d_assoc and k_ndt_pyr_solve: a slot at level l has the bits of an iteration of
// sps_ndt_align_d2d on that level.  The rules of those files hold unchanged (float64, contraction off, loc_mul / loc_add /
// __ddiv_rn, no float atomics, their integer atomics, plain vector stores).
//
// The scratch of the source build is array-major (ndt_src_layout, ndt_d2d_host.inc.h): every array holds all levels back to
// back and a level's slice is the array's base plus level x stride.  The per-level resolution and min_points are a small
// by-value struct selected by value, as k_ndt_pyr_solve selects its caps: a by-value array indexed by the level would live
// in scratch memory.  The thinned points do not depend on the level: every level's lookup forms them (the identity pose),
// level 0 alone stores them, and all levels' stats launches read that one array.

#pragma clang fp contract(off)

struct NdtPyrSrcParams {
  double resolution[NDT_PYR_MAX];   // edge of a level's source cells
  int min_points[NDT_PYR_MAX];      // points from which a level's cell is valid
};

__device__ inline double ndt_pyr_src_resolution(const NdtPyrSrcParams &p, int l) {
  return l == 0 ? p.resolution[0] : (l == 1 ? p.resolution[1] : (l == 2 ? p.resolution[2] : p.resolution[3]));
}
__device__ inline int ndt_pyr_src_min_points(const NdtPyrSrcParams &p, int l) {
  return l == 0 ? p.min_points[0] : (l == 1 ? p.min_points[1] : (l == 2 ? p.min_points[2] : p.min_points[3]));
}

// level l's empty map and its state from level 0's (w: the entries of one level's per-point arrays and of its hashes)
__device__ inline NdtMap ndt_pyr_src_map(NdtMap m, int l, const NdtPyrUpdStride &w, double resolution) {
  const size_t ph = (size_t)l * (size_t)w.hs;
  m.h.keys += ph, m.h.rank += ph;
  m.resolution = resolution;
  return m;
}
__device__ inline NdtDyn ndt_pyr_src_dyn(NdtDyn d, int l, const NdtPyrUpdStride &w) {
  const size_t pn = (size_t)l * (size_t)w.n;
  d.keys += pn, d.bcnt += pn, d.lead += pn, d.cstart += pn;
  d.state += 4 * l;
  return d;
}

// ---- the scan's cells at every level: the blocks of one level in x, the levels in y -----------------------------------------
__global__ __launch_bounds__(256) void k_ndt_pyr_src_lookup(const double *__restrict__ pts, const int *__restrict__ n_dev, int cap,
                                                             LocPose Th, NdtMap m0, NdtUpdScratch s0, NdtPyrUpdStride w,
                                                             NdtPyrSrcParams p) {
  const int l = blockIdx.y;
  ndt_upd_lookup_body(pts, n_dev, cap, Th, nullptr, nullptr, ndt_pyr_src_map(m0, l, w, ndt_pyr_src_resolution(p, l)),
                      ndt_pyr_upd_slice(s0, l, w), l == 0);
}
__global__ __launch_bounds__(NDT_UPD_BLOCK) void k_ndt_pyr_src_found(const int *__restrict__ n_dev, int cap, NdtDyn d0,
                                                                      NdtUpdScratch s0, NdtPyrUpdStride w, int *__restrict__ info) {
  __shared__ int lds[NDT_UPD_BLOCK / 64];
  const int l = blockIdx.y;
  ndt_upd_found_body(n_dev, cap, nullptr, ndt_pyr_src_dyn(d0, l, w), ndt_pyr_upd_slice(s0, l, w), info + 4 * l, lds);
}
__global__ __launch_bounds__(256) void k_ndt_pyr_src_resolve(const int *__restrict__ n_dev, int cap, NdtMap m0, NdtDyn d0,
                                                              NdtUpdScratch s0, NdtPyrUpdStride w, NdtPyrSrcParams p) {
  const int l = blockIdx.y;
  ndt_upd_resolve_body(n_dev, cap, nullptr, ndt_pyr_src_map(m0, l, w, ndt_pyr_src_resolution(p, l)), ndt_pyr_src_dyn(d0, l, w),
                       ndt_pyr_upd_slice(s0, l, w));
}
__global__ __launch_bounds__(NDT_UPD_BLOCK) void k_ndt_pyr_src_offsets(const int *__restrict__ n_dev, int cap, NdtDyn d0,
                                                                        NdtUpdScratch s0, NdtPyrUpdStride w,
                                                                        int *__restrict__ info) {
  __shared__ int lds[NDT_UPD_BLOCK / 64];
  const int l = blockIdx.y;
  ndt_upd_offsets_body(n_dev, cap, nullptr, ndt_pyr_src_dyn(d0, l, w), ndt_pyr_upd_slice(s0, l, w), info + 4 * l, lds);
}
__global__ __launch_bounds__(256) void k_ndt_pyr_src_fill(const int *__restrict__ n_dev, int cap, NdtDyn d0, NdtUpdScratch s0,
                                                           NdtPyrUpdStride w) {
  const int l = blockIdx.y;
  ndt_upd_fill_body(n_dev, cap, nullptr, ndt_pyr_src_dyn(d0, l, w), ndt_pyr_upd_slice(s0, l, w));
}
__global__ __launch_bounds__(64) void k_ndt_pyr_src_stats(const int *__restrict__ n_dev, int cap, NdtDyn d0, NdtUpdScratch s0,
                                                           NdtPyrUpdStride w) {
  __shared__ unsigned bits[NDT_UPD_MAX_POINTS / 32];
  const int l = blockIdx.y;
  ndt_upd_stats_body(n_dev, cap, nullptr, ndt_pyr_src_dyn(d0, l, w), ndt_pyr_upd_slice(s0, l, w), bits);
}
// src [L][cap][NDT_SRC_REC], src_count [L][cap] (may be null), n_src [L][2] (zero on entry: the host's memset)
__global__ __launch_bounds__(256) void k_ndt_pyr_src_records(const int *__restrict__ n_dev, int cap, NdtPyrSrcParams p,
                                                              double eig_ratio, NdtUpdScratch s0, NdtPyrUpdStride w,
                                                              double *__restrict__ src, int *__restrict__ src_count,
                                                              int *__restrict__ n_src) {
  const int l = blockIdx.y;
  const size_t row = (size_t)l * (size_t)cap;
  ndt_src_records_body(n_dev, cap, ndt_pyr_src_min_points(p, l), eig_ratio, ndt_pyr_upd_slice(s0, l, w), src + row * NDT_SRC_REC,
                       src_count ? src_count + row : nullptr, n_src + 2 * l);
}

// ---- alignment -------------------------------------------------------------------------------------------------------------
// Launch A.  Grid and workgroup of k_ndt_d2d_assoc.  The level is the same for every thread of the grid: it goes through a
// scalar register, and the level's descriptor is read from the pyramid's device array, as in k_ndt_pyr_assoc.
__global__ __launch_bounds__(256) void k_ndt_d2d_pyr_assoc(const double *__restrict__ src, const int *__restrict__ n_src, int cap,
                                                            const NdtPyrLevel *__restrict__ levels, int n_levels, int neighbours,
                                                            const double *__restrict__ T, const int *__restrict__ state,
                                                            double *__restrict__ partial) {
  __shared__ NdtAssocLds lds;
  if (state[0]) return;
  const int l = __builtin_amdgcn_readfirstlane(min(max(state[1], 0), n_levels - 1));
  const NdtPyrLevel d = levels[l];
  ndt_d2d_assoc_body(src + (size_t)l * (size_t)cap * NDT_SRC_REC, n_src + 2 * l, cap, d.m, d.gs, neighbours, T, partial, lds);
}

// The level that follows l: the next one whose valid sources, clipped to cap, are at least min_corr; < 0 where there is none
// and l is the last.  A level below that bound could only end the call with status 2.
__device__ inline int ndt_d2d_pyr_next(const int *__restrict__ n_src, int cap, int l, int n_levels, int min_corr) {
  for (int k = l + 1; k < n_levels; ++k)
    if (min(cap, max(n_src[2 * k + 1], 0)) >= min_corr) return k;
  return -1;
}

// Launch B, one workgroup of 256: k_ndt_pyr_solve with the rows of the current level's sources and the handoff above.
__global__ __launch_bounds__(256) void k_ndt_d2d_pyr_solve(const double *__restrict__ partial, const int *__restrict__ n_src,
                                                            int cap, int slot, int n_levels, NdtPyrCaps caps, int min_corr,
                                                            double tol_t, double tol_r, LocPose T_init, double *__restrict__ T,
                                                            int *__restrict__ status, int *__restrict__ state,
                                                            double *__restrict__ trace, double *__restrict__ normal,
                                                            int *__restrict__ level) {
  __shared__ double seg[LOC_SEG][32];
  __shared__ double tot[32];
  if (state[0]) return;
  const int l = min(max(state[1], 0), n_levels - 1);
  const int n = min(cap, max(n_src[2 * l], 0));
  ndt_pyr_solve_body(partial, n, slot, l, ndt_d2d_pyr_next(n_src, cap, l, n_levels, min_corr), caps, min_corr, tol_t, tol_r,
                     T_init, T, status, state, trace, normal, level, seg, tot);
}

#pragma clang fp contract(fast)
