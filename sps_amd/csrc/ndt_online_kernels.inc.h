// ndt_online_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after
// ndt_pyramid_kernels.inc.h): the kernels of the online NDT maps, the single map and the pyramid alike (host side:
// ndt_online_host.inc.h; ABI: the "NDT localiser, online map", "... free-space carving" and "... online pyramid" sections
// of include/sps_hip.h).  The single map of a context is a pyramid of one level: gridDim.y = 1.
//
//   k_ndt_upd_lookup .. k_ndt_upd_merge        the seven launches of the update, grid (blocks of one level, levels)
//   k_ndt_carve_begin / _rays / _decide        the three launches of the carve, the same grid shape
//
// Nothing is computed here: every kernel picks its level, blockIdx.y, and calls its body of ndt_update_kernels.inc.h /
// ndt_carve_kernels.inc.h with that level's map, state, scratch slice and info words.  So level l of L gets the bits of a
// launch with that level alone, and the rules of those files hold unchanged (float64, contraction off, loc_mul / loc_add /
// __ddiv_rn, no float atomics, their integer atomics, plain vector stores).
//
// The level is uniform per workgroup and already scalar.  A level's descriptors (NdtPyrLevel, NdtDyn) come from the two
// device arrays of the pyramid by scalar loads; a by-value kernel-argument array indexed by the level would live in
// scratch.  The scratch of the caller is array-major (ndt_pyr_upd_layout): every array holds all levels back to back, a
// level's slice is the array's base plus level x stride, and the stride is the same for every level because `cap` is.
// The transformed points q do not depend on the level: every level's lookup forms them in registers, level 0 alone stores
// them, and all levels' stats launches read that one array.  Per-call per-level scalars (the carve's end margins) are a
// small by-value struct selected by value, as k_ndt_pyr_solve selects its caps.

#pragma clang fp contract(off)

// what turns the level-0 scratch into the slice of level l: the points and the hash slots of one level
struct NdtPyrUpdStride {
  int n;                   // max(cap, 1): entries of the per-point arrays of one level
  int hs;                  // slots of one level's update hash
};

struct NdtPyrMargins {
  double v[NDT_PYR_MAX];   // the carve's end margin of every level
};

__device__ inline NdtUpdScratch ndt_pyr_upd_slice(NdtUpdScratch s, int l, const NdtPyrUpdStride &w) {
  const size_t pn = (size_t)l * (size_t)w.n, ph = (size_t)l * (size_t)w.hs;
  s.bstat += pn * 10;
  s.cell_of += pn, s.slot_of += pn, s.list += pn, s.tcell += pn;
  s.n_touched += l;
  s.h.keys += ph, s.h.first += ph, s.h.rank += ph;
  return s;   // s.q is shared by the levels
}

__device__ inline double ndt_pyr_margin(const NdtPyrMargins &e, int l) {
  return l == 0 ? e.v[0] : (l == 1 ? e.v[1] : (l == 2 ? e.v[2] : e.v[3]));
}

// ---- the update: the blocks of one level in x, the levels in y -------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ndt_upd_lookup(const double *__restrict__ pts, const int *__restrict__ n_dev, int cap,
                                                         LocPose Th, const double *__restrict__ T_dev,
                                                         const int *__restrict__ gate, const NdtPyrLevel *__restrict__ levels,
                                                         NdtUpdScratch s0, NdtPyrUpdStride w) {
  const int l = blockIdx.y;
  const NdtMap m = levels[l].m;
  ndt_upd_lookup_body(pts, n_dev, cap, Th, T_dev, gate, m, ndt_pyr_upd_slice(s0, l, w), l == 0);
}

__global__ __launch_bounds__(NDT_UPD_BLOCK) void k_ndt_upd_found(const int *__restrict__ n_dev, int cap,
                                                                  const int *__restrict__ gate, const NdtDyn *__restrict__ dyn,
                                                                  NdtUpdScratch s0, NdtPyrUpdStride w, int *__restrict__ info) {
  __shared__ int lds[NDT_UPD_BLOCK / 64];
  const int l = blockIdx.y;
  const NdtDyn d = dyn[l];
  ndt_upd_found_body(n_dev, cap, gate, d, ndt_pyr_upd_slice(s0, l, w), info + 4 * l, lds);
}

__global__ __launch_bounds__(256) void k_ndt_upd_resolve(const int *__restrict__ n_dev, int cap, const int *__restrict__ gate,
                                                          const NdtPyrLevel *__restrict__ levels, const NdtDyn *__restrict__ dyn,
                                                          NdtUpdScratch s0, NdtPyrUpdStride w) {
  const int l = blockIdx.y;
  const NdtMap m = levels[l].m;
  const NdtDyn d = dyn[l];
  ndt_upd_resolve_body(n_dev, cap, gate, m, d, ndt_pyr_upd_slice(s0, l, w));
}

__global__ __launch_bounds__(NDT_UPD_BLOCK) void k_ndt_upd_offsets(const int *__restrict__ n_dev, int cap,
                                                                    const int *__restrict__ gate, const NdtDyn *__restrict__ dyn,
                                                                    NdtUpdScratch s0, NdtPyrUpdStride w, int *__restrict__ info) {
  __shared__ int lds[NDT_UPD_BLOCK / 64];
  const int l = blockIdx.y;
  const NdtDyn d = dyn[l];
  ndt_upd_offsets_body(n_dev, cap, gate, d, ndt_pyr_upd_slice(s0, l, w), info + 4 * l, lds);
}

__global__ __launch_bounds__(256) void k_ndt_upd_fill(const int *__restrict__ n_dev, int cap, const int *__restrict__ gate,
                                                       const NdtDyn *__restrict__ dyn, NdtUpdScratch s0, NdtPyrUpdStride w) {
  const int l = blockIdx.y;
  const NdtDyn d = dyn[l];
  ndt_upd_fill_body(n_dev, cap, gate, d, ndt_pyr_upd_slice(s0, l, w));
}

__global__ __launch_bounds__(64) void k_ndt_upd_stats(const int *__restrict__ n_dev, int cap, const int *__restrict__ gate,
                                                       const NdtDyn *__restrict__ dyn, NdtUpdScratch s0, NdtPyrUpdStride w) {
  __shared__ unsigned bits[NDT_UPD_MAX_POINTS / 32];
  const int l = blockIdx.y;
  const NdtDyn d = dyn[l];
  ndt_upd_stats_body(n_dev, cap, gate, d, ndt_pyr_upd_slice(s0, l, w), bits);
}

__global__ __launch_bounds__(256) void k_ndt_upd_merge(const int *__restrict__ n_dev, int cap, const int *__restrict__ gate,
                                                        int max_cell_points, const NdtDyn *__restrict__ dyn, NdtUpdScratch s0,
                                                        NdtPyrUpdStride w) {
  const int l = blockIdx.y;
  const NdtDyn d = dyn[l];
  ndt_upd_merge_body(n_dev, cap, gate, max_cell_points, d, ndt_pyr_upd_slice(s0, l, w));
}

// ---- the carve: gridDim.x covers the largest capacity (begin, decide) or the points (rays); the surplus blocks of a
// smaller level find their cell index at or past its capacity and do nothing ------------------------------------------------
__global__ __launch_bounds__(256) void k_ndt_carve_begin(const int *__restrict__ gate, const NdtDyn *__restrict__ dyn,
                                                          int *__restrict__ info) {
  const int l = blockIdx.y;
  const NdtDyn d = dyn[l];
  ndt_carve_begin_body(gate, d, info + 4 * l);
}

__global__ __launch_bounds__(256) void k_ndt_carve_rays(const double *__restrict__ pts, const int *__restrict__ n_dev, int cap,
                                                         LocPose Th, const double *__restrict__ T_dev,
                                                         const int *__restrict__ gate, const NdtPyrLevel *__restrict__ levels,
                                                         const NdtDyn *__restrict__ dyn, NdtCarveParams p, NdtPyrMargins e,
                                                         int *__restrict__ info) {
  const int l = blockIdx.y;
  const NdtMap m = levels[l].m;
  const NdtDyn d = dyn[l];
  p.end_margin = ndt_pyr_margin(e, l);
  ndt_carve_rays_body(pts, n_dev, cap, Th, T_dev, gate, m, d, p, info + 4 * l);
}

__global__ __launch_bounds__(256) void k_ndt_carve_decide(const int *__restrict__ gate, const NdtDyn *__restrict__ dyn,
                                                           NdtCarveParams p, int *__restrict__ info) {
  const int l = blockIdx.y;
  const NdtDyn d = dyn[l];
  ndt_carve_decide_body(gate, d, p, info + 4 * l);   // the decision reads no end margin
}

#pragma clang fp contract(fast)
