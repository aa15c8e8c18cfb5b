// ndt_d2d_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after ndt_update_kernels.inc.h):
// distribution-to-distribution NDT (host side: ndt_d2d_host.inc.h; ABI: the "NDT localiser, distribution to distribution"
// section of include/sps_hip.h).  The scan is reduced to Gaussians too, one per cell of the sensor frame, and
// those are registered against the map's.
//
//   (source build, 1 - 6)  the bodies of the online update, ndt_update_kernels.inc.h, run against an empty map of capacity
//                          `cap` that lives in the caller's scratch, at the identity pose: every cell of the scan is
//                          founded, cell id = rank of its lowest point, and k_ndt_upd_stats leaves n, mean and S per cell
//                          in bstat, cells in that order, points in ascending index
//   k_ndt_src_records      (source build, 7)  one thread per cell: ndt_floored_eigen, covariance, flag -> one 80-byte record
//                          (its body is ndt_src_records_body, which ndt_d2d_pyramid_kernels.inc.h runs once per level)
//   k_ndt_d2d_assoc        (launch A of an iteration)  q = R mu + t, Cw = R C R^T, the records of q's cell and its face
//                          neighbours, per cell B = inv3(inv3(icov) + Cw) and the normal-equation terms with B
//                          (its body is ndt_d2d_assoc_body, which ndt_d2d_batch_kernels.inc.h runs once per hypothesis)
//
// Launch B is k_loc_solve unchanged.  The rules of ndt_kernels.inc.h hold: float64, contraction off, loc_mul / loc_add /
// __ddiv_rn, no float atomics, no sum that depends on the order in which threads arrive.  The one atomic of this file is an
// integer atomicAdd that counts valid records.

#pragma clang fp contract(off)

constexpr int NDT_SRC_REC = 10;   // doubles of a source record: mean[3], cov[6] (xx, xy, xz, yy, yz, zz), valid (1.0 / 0.0)
static_assert(NDT_SRC_REC == SPS_NDT_SRC_REC, "the source record of the ABI");

// ---- the scan's cells -------------------------------------------------------------------------------------------------
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

// 7: one thread per cell t (bstat row t: n, mean, S).  The covariance is reassembled from the floored eigenvalues, entry
// (i, j) = ((v_i0 v_j0) l0 + (v_i1 v_j1) l1) + (v_i2 v_j2) l2.  n_src[0] = cells (thread 0), n_src[1] counts the valid ones
// (zero on entry: the host's memset).  The body indexes by blockIdx.x only: k_ndt_pyr_src_records
// (ndt_d2d_pyramid_kernels.inc.h) runs it once per level of a pyramid of sources.
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

// Launch A.  NDT_LANES lanes per source cell, LOC_PTS sources per workgroup; the geometry and the LDS of k_ndt_assoc.
//   phase 1: every lane of a valid source forms q and Cw (the same values on its eight lanes: they share a wave, so forming
//            them once and passing them on would save no time); lane c < neighbours looks up cell c of q (ndt_cell_of) and,
//            where the cell contributes (ndt_d2d_hit), leaves a = -d1 w, B, y = B x and the score in LDS;
//   phases 2 and 3: ndt_assoc_reduce, with B where k_ndt_assoc has the cell's inverse covariance.
// A source that is not valid, or lies beyond the cells built, contributes nothing and is not counted.
// The body is shared with k_ndt_d2d_assoc_batch (ndt_d2d_batch_kernels.inc.h), which runs it once per hypothesis: T is the
// pose, partial the rows of that pose, blockIdx.x the workgroup's place among them.
__device__ inline void ndt_d2d_assoc_body(const double *__restrict__ src, const int *__restrict__ n_src, int cap, const NdtMap &m,
                                          const NdtGauss &gs, int neighbours, const double *__restrict__ T,
                                          double *__restrict__ partial, NdtAssocLds &lds) {
  const int n = min(cap, max(*n_src, 0));
  const int base = blockIdx.x * LOC_PTS;
  if (base >= n) return;
  const int k = threadIdx.x / NDT_LANES, sub = threadIdx.x % NDT_LANES;
  const int i = base + k;
  double q[3] = {0.0, 0.0, 0.0};
  int ok = 0;
  if (i < n) {
    double s[NDT_SRC_REC];
#pragma unroll
    for (int j = 0; j < NDT_SRC_REC; ++j) s[j] = src[(size_t)i * NDT_SRC_REC + j];
    if (s[9] != 0.0) {
      loc_transform(T, s[0], s[1], s[2], q);
      double Cw[6];
      ndt_rotate_cov(T, s + 3, Cw);
      const int cell = sub < neighbours ? ndt_cell_of(m, q, sub) : -1;
      double e, w, y[3], B[6];
      if (cell >= 0 && ndt_d2d_hit(q, Cw, m.rec + (size_t)cell * NDT_REC, gs, e, w, y, B)) {
        double *o = lds.hit[k][sub];
        o[0] = loc_mul(gs.nd1, w);
#pragma unroll
        for (int j = 0; j < 6; ++j) o[1 + j] = B[j];
        o[7] = y[0], o[8] = y[1], o[9] = y[2];
        o[10] = loc_mul(gs.nd1, e);
        ok = 1;
      }
    }
  }
  lds.hit_ok[k][sub] = ok;
  ndt_assoc_reduce(lds, k, sub, q, neighbours, partial);
}

__global__ __launch_bounds__(256) void k_ndt_d2d_assoc(const double *__restrict__ src, const int *__restrict__ n_src, int cap,
                                                        NdtMap m, NdtGauss gs, int neighbours, const double *__restrict__ T,
                                                        const int *__restrict__ done, double *__restrict__ partial) {
  __shared__ NdtAssocLds lds;
  if (*done) return;
  ndt_d2d_assoc_body(src, n_src, cap, m, gs, neighbours, T, partial, lds);
}

#pragma clang fp contract(fast)
