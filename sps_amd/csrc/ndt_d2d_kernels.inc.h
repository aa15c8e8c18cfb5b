// ndt_d2d_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after ndt_online_kernels.inc.h):
// distribution-to-distribution NDT (host side: ndt_d2d_host.inc.h; ABI: the "NDT localiser, distribution to distribution"
// sections of include/sps_hip.h).  The scan is reduced to Gaussians too, one per cell of the sensor
// frame, at one resolution or at one per level of a pyramid, and those are registered against the map's.
//
//   k_ndt_src_lookup .. k_ndt_src_stats   (source build, 1 - 6)  the bodies of the online update, ndt_update_kernels.inc.h, run
//                          against an empty map of capacity `cap` that lives in the caller's scratch, at the identity pose:
//                          every cell of the scan is founded, cell id = rank of its lowest point, and k_ndt_src_stats leaves
//                          n, mean and S per cell in bstat, cells in that order, points in ascending index
//   k_ndt_src_records      (source build, 7)  one thread per cell: ndt_floored_eigen, covariance, flag -> one 80-byte record
//   k_ndt_pyr_src_*        the same seven for a pyramid of sources, grid (blocks of one level, levels)
//   k_ndt_d2d_assoc        launch A of sps_ndt_align_d2d: ndt_assoc_body of NdtCells
//   NdtCells               the scan's cells as the policy type of launch A's body, of the batch's and the pyramid's launches
//                          and of the scorer (k_ndt_assoc_batch, k_ndt_pyr_assoc, k_ndt_pyr_solve, k_ndt_score: templates over
//                          the scan): q = R mu + t, Cw = R C R^T, the records of q's cell and its face neighbours, per cell
//                          B = inv3(inv3(icov) + Cw) and the normal-equation terms with B
//
// The single build keeps its seven by-value kernels: through the level-in-grid kernels at one level, three builds in a row
// read 1 % slower in two sessions (profiles/ndt_one_scan).  The pyramid's source kernels compute nothing: they
// pick their level, blockIdx.y, and call the bodies of ndt_update_kernels.inc.h and ndt_src_records_body with that level's
// slice of the scratch, as ndt_online_kernels.inc.h does for the online maps, so level l of L has the bits of a build with
// that level alone.  The scratch is array-major (ndt_src_layout, ndt_d2d_host.inc.h): every array holds all levels back to
// back and a level's slice is the array's base plus level x stride.  The per-level resolution and min_points are a small
// by-value struct selected by value, as k_ndt_pyr_solve selects its caps: a by-value array indexed by the level would live
// in scratch memory.  The thinned points do not depend on the level: every level's lookup forms them (the identity pose),
// level 0 alone stores them, and all levels' stats launches read that one array.
//
// Launch B, the initialisation, the select and the scorer's second launch are k_loc_solve, k_loc_init*, k_ndt_select and
// k_ndt_score_reduce unchanged: all of them take their row count from the count they are handed, which here is the source
// count.  The rules of ndt_kernels.inc.h hold: float64, contraction off, loc_mul / loc_add / __ddiv_rn, no float atomics, no
// sum that depends on the order in which threads arrive.  The one atomic of this file is an integer atomicAdd that counts
// valid records.

#pragma clang fp contract(off)

constexpr int NDT_SRC_REC = 10;   // doubles of a source record: mean[3], cov[6] (xx, xy, xz, yy, yz, zz), valid (1.0 / 0.0)
static_assert(NDT_SRC_REC == SPS_NDT_SRC_REC, "the source record of the ABI");

// ---- the scan's cells, one level (sps_ndt_source_build) ---------------------------------------------------------------
// the update's kernels 1 to 6 with nothing but their bodies' arguments: the map is the empty one of the scratch, the pose
// the identity (Th), there is no device pose and no gate
__global__ __launch_bounds__(256) void k_ndt_src_lookup(const double *__restrict__ pts, const int *__restrict__ n_dev, int cap,
                                                         LocPose Th, NdtMap m, NdtUpdScratch s) {
  ndt_upd_lookup_body(pts, n_dev, cap, Th, nullptr, nullptr, m, s, true);
}
__global__ __launch_bounds__(NDT_UPD_BLOCK) void k_ndt_src_found(const int *__restrict__ n_dev, int cap, NdtDyn d, NdtUpdScratch s,
                                                                  int *__restrict__ info) {
  __shared__ int lds[NDT_UPD_BLOCK / 64];
  ndt_upd_found_body(n_dev, cap, nullptr, d, s, info, lds);
}
__global__ __launch_bounds__(256) void k_ndt_src_resolve(const int *__restrict__ n_dev, int cap, NdtMap m, NdtDyn d,
                                                          NdtUpdScratch s) {
  ndt_upd_resolve_body(n_dev, cap, nullptr, m, d, s);
}
__global__ __launch_bounds__(NDT_UPD_BLOCK) void k_ndt_src_offsets(const int *__restrict__ n_dev, int cap, NdtDyn d,
                                                                    NdtUpdScratch s, int *__restrict__ info) {
  __shared__ int lds[NDT_UPD_BLOCK / 64];
  ndt_upd_offsets_body(n_dev, cap, nullptr, d, s, info, lds);
}
__global__ __launch_bounds__(256) void k_ndt_src_fill(const int *__restrict__ n_dev, int cap, NdtDyn d, NdtUpdScratch s) {
  ndt_upd_fill_body(n_dev, cap, nullptr, d, s);
}
__global__ __launch_bounds__(64) void k_ndt_src_stats(const int *__restrict__ n_dev, int cap, NdtDyn d, NdtUpdScratch s) {
  __shared__ unsigned bits[NDT_UPD_MAX_POINTS / 32];
  ndt_upd_stats_body(n_dev, cap, nullptr, d, s, bits);
}

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
// the update's kernels 1 to 6 with nothing but their bodies' arguments: the map is the empty one of the scratch, the pose
// the identity (Th), there is no device pose and no gate
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
// 7: one thread per cell t (bstat row t: n, mean, S).  The covariance is reassembled from the floored eigenvalues, entry
// (i, j) = ((v_i0 v_j0) l0 + (v_i1 v_j1) l1) + (v_i2 v_j2) l2.  n_src[0] = cells (thread 0), n_src[1] counts the valid ones
// (zero on entry: the host's memset).  The body indexes by blockIdx.x only: k_ndt_pyr_src_records runs it once per level.
__device__ inline void ndt_src_records_body(const int *__restrict__ n_dev, int cap, int min_points, double eig_ratio,
                                            const NdtUpdScratch &s, double *__restrict__ src, int *__restrict__ src_count,
                                            int *__restrict__ n_src) {
  const int nt = min(max(*s.n_touched, 0), min(cap, max(*n_dev, 0)));
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t == 0) n_src[0] = nt;
  if (t >= nt) return;
  const double *b = s.bstat + (size_t)t * 10;
  const int n = (int)b[0];
  const double mu[3] = {b[1], b[2], b[3]};
  double cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool valid = n >= min_points && n >= 2;
  if (n >= 2) {
    double v[3][3], lam[3], lmax;
    ndt_floored_eigen(n, b + 4, eig_ratio, v, lam, lmax);
    valid = valid && lmax > 0.0;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j, ++k)
        cov[k] = loc_add(loc_add(loc_mul(loc_mul(v[i][0], v[j][0]), lam[0]), loc_mul(loc_mul(v[i][1], v[j][1]), lam[1])),
                         loc_mul(loc_mul(v[i][2], v[j][2]), lam[2]));
  }
  for (int a = 0; a < 3; ++a) valid = valid && isfinite(mu[a]);
  for (int i = 0; i < 6; ++i) valid = valid && isfinite(cov[i]);
  double *o = src + (size_t)t * NDT_SRC_REC;
  o[0] = mu[0], o[1] = mu[1], o[2] = mu[2];
#pragma unroll
  for (int i = 0; i < 6; ++i) o[3 + i] = cov[i];
  o[9] = valid ? 1.0 : 0.0;
  if (src_count) src_count[t] = n;
  if (valid) atomicAdd(&n_src[1], 1);
}

__global__ __launch_bounds__(256) void k_ndt_src_records(const int *__restrict__ n_dev, int cap, int min_points, double eig_ratio,
                                                          NdtUpdScratch s, double *__restrict__ src, int *__restrict__ src_count,
                                                          int *__restrict__ n_src) {
  ndt_src_records_body(n_dev, cap, min_points, eig_ratio, s, src, src_count, n_src);
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

// ---- alignment -------------------------------------------------------------------------------------------------------
// The inverse of the symmetric 3 x 3 matrix m (xx, xy, xz, yy, yz, zz) by cofactors, every entry a true division by
// det = (m0 c00 + m1 c01) + m2 c02.  False where det <= 0 (NaN included) or an entry is not finite.
__device__ inline bool ndt_inv3(const double m[6], double o[6]) {
  const double c00 = loc_add(loc_mul(m[3], m[5]), -loc_mul(m[4], m[4]));
  const double c01 = loc_add(loc_mul(m[2], m[4]), -loc_mul(m[1], m[5]));
  const double c02 = loc_add(loc_mul(m[1], m[4]), -loc_mul(m[2], m[3]));
  const double c11 = loc_add(loc_mul(m[0], m[5]), -loc_mul(m[2], m[2]));
  const double c12 = loc_add(loc_mul(m[1], m[2]), -loc_mul(m[0], m[4]));
  const double c22 = loc_add(loc_mul(m[0], m[3]), -loc_mul(m[1], m[1]));
  const double det = loc_add(loc_add(loc_mul(m[0], c00), loc_mul(m[1], c01)), loc_mul(m[2], c02));
  if (!(det > 0.0)) return false;
  o[0] = __ddiv_rn(c00, det), o[1] = __ddiv_rn(c01, det), o[2] = __ddiv_rn(c02, det);
  o[3] = __ddiv_rn(c11, det), o[4] = __ddiv_rn(c12, det), o[5] = __ddiv_rn(c22, det);
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 6; ++i) finite = finite && isfinite(o[i]);
  return finite;
}

// Cw = R C R^T (six upper entries) for the rotation of the pose T and the symmetric C: U = R C first, every entry
// (a0 b0 + a1 b1) + a2 b2, then Cw = U R^T the same way
__device__ inline void ndt_rotate_cov(const double *T, const double C[6], double Cw[6]) {
  double U[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double r[3] = {T[4 * i], T[4 * i + 1], T[4 * i + 2]};
#pragma unroll
    for (int j = 0; j < 3; ++j) U[i][j] = ndt_symrow(C, j, r);   // sum_k R[i][k] C[k][j]: column j of C is its row j
  }
  int k = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j, ++k) {
      const double r[3] = {T[4 * j], T[4 * j + 1], T[4 * j + 2]};
      Cw[k] = loc_dot3(U[i], r);
    }
}

// One map cell's contribution to the source (q, Cw): Sm = inv3(icov), M = Sm + Cw, B = inv3(M), x = q - mean, y = B x,
// e = exp(-d2 x.y / 2), w = d2 e.  False where the record is not valid, an inverse fails or w fails the guard of
// ndt_cell_hit.
__device__ inline bool ndt_d2d_hit(const double q[3], const double Cw[6], const double *__restrict__ rec, const NdtGauss &gs,
                                   double &e, double &w, double y[3], double B[6]) {
  double r[NDT_REC];
#pragma unroll
  for (int j = 0; j < NDT_REC; ++j) r[j] = rec[j];
  if (r[9] == 0.0) return false;
  double Sm[6], M[6];
  if (!ndt_inv3(r + 3, Sm)) return false;
#pragma unroll
  for (int j = 0; j < 6; ++j) M[j] = loc_add(Sm[j], Cw[j]);
  if (!ndt_inv3(M, B)) return false;
  const double x[3] = {loc_add(q[0], -r[0]), loc_add(q[1], -r[1]), loc_add(q[2], -r[2])};
#pragma unroll
  for (int a = 0; a < 3; ++a) y[a] = ndt_symrow(B, a, x);
  e = exp(loc_mul(-0.5, loc_mul(gs.d2, loc_dot3(x, y))));
  w = loc_mul(gs.d2, e);
  return w >= 0.0 && w <= 1.0;
}

// The scan's cells as the scan of launch A (the policy type described in ndt_kernels.inc.h).  Every lane of a valid source
// forms q and Cw (the same values on its eight lanes: they share a wave, so forming them once and passing them on would
// save no time).  A source that is not valid, or lies beyond the cells built, contributes nothing and is not counted.  In a
// pyramid level l's records are the slice src + l * cap * NDT_SRC_REC and its counts n_src[2 l] (cells) and n_src[2 l + 1]
// (valid cells); the level that follows l is the next one whose valid sources, clipped to cap, are at least min_corr: a
// level below that bound could only end the call with status 2.
struct NdtCells {
  static constexpr int ELEM = NDT_SRC_REC;
  __device__ static bool valid(const double *s) { return s[9] != 0.0; }
  __device__ static bool hit(const NdtMap &m, const NdtGauss &gs, const double *T, const double *s, int sub, int neighbours,
                             double q[3], double &e, double &w, double y[3], double B[6]) {
    loc_transform(T, s[0], s[1], s[2], q);
    double Cw[6];
    ndt_rotate_cov(T, s + 3, Cw);
    const int cell = sub < neighbours ? ndt_cell_of(m, q, sub) : -1;
    return cell >= 0 && ndt_d2d_hit(q, Cw, m.rec + (size_t)cell * NDT_REC, gs, e, w, y, B);
  }
  __device__ static const double *level_elems(const double *src, int cap, int l) {
    return src + (size_t)l * (size_t)cap * NDT_SRC_REC;
  }
  __device__ static const int *level_count(const int *n_src, int l) { return n_src + 2 * l; }
  __device__ static int next(const int *n_src, int cap, int l, int n_levels, int min_corr) {
    for (int k = l + 1; k < n_levels; ++k)
      if (min(cap, max(n_src[2 * k + 1], 0)) >= min_corr) return k;
    return -1;
  }
  // where the chain of `next` from level 0 ends: the last level that is not skipped, 0 where every other one is
  __device__ static int last(const int *n_src, int cap, int n_levels, int min_corr) {
    int l = 0;
    for (int k = 1; k < n_levels; ++k)
      if (min(cap, max(n_src[2 * k + 1], 0)) >= min_corr) l = k;
    return l;
  }
};

// launch A of sps_ndt_align_d2d: k_ndt_assoc (ndt_kernels.inc.h) for the scan's cells
__global__ __launch_bounds__(256) void k_ndt_d2d_assoc(const double *__restrict__ src, const int *__restrict__ n_src, int cap,
                                                        NdtMap m, NdtGauss gs, int neighbours, const double *__restrict__ T,
                                                        const int *__restrict__ done, double *__restrict__ partial) {
  __shared__ NdtAssocLds lds;
  if (*done) return;
  ndt_assoc_body<NdtCells>(src, n_src, cap, m, gs, neighbours, T, partial, lds);
}

#pragma clang fp contract(fast)
