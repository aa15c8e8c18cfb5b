// loc_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace): the scan-to-map localiser
// (host side: loc_host.inc.h; ABI: the "localiser" section of include/sps_hip.h).
//
//   k_loc_ds_insert / k_loc_ds_count / k_loc_ds_write   voxel-grid thinning of the kept rows (lowest row index per voxel)
//   k_loc_init                                          T_out = T_init, status = (1, 0, 0, 0), done = 0
//   k_loc_assoc   (launch A of an iteration)            nearest map point of every scan point + the normal-equation terms
//   k_loc_solve   (launch B of an iteration)            ordered sum, 6x6 Cholesky, Rodrigues, pose update, status
//
// A deterministic point-to-point ICP: no float atomics; every float sum goes through per-workgroup partial rows that
// are combined in block order; the only atomic is an integer atomicMin whose result does not depend on arrival order.
// All geometry is float64 and every operation is rounded on its own, so a host restatement that does the same agrees
// step by step.  The compiler contracts a * b + c into an FMA by default, also through __dmul_rn / __dadd_rn (plain
// * and + in the HIP headers), so this file switches contraction off for its own code and spells the products and
// sums through loc_mul / loc_add.

#pragma clang fp contract(off)
__device__ inline double loc_mul(double a, double b) { return a * b; }
__device__ inline double loc_add(double a, double b) { return a + b; }

// q = R p + t of the pose T (row-major, its first 12 entries), per axis ((T0 px + T1 py) + T2 pz) + T3: the one definition
// behind k_loc_assoc and every NDT kernel that moves a scan point into the map frame
__device__ inline void loc_transform(const double *T, double px, double py, double pz, double q[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
    q[a] = loc_add(loc_add(loc_add(loc_mul(T[4 * a], px), loc_mul(T[4 * a + 1], py)), loc_mul(T[4 * a + 2], pz)), T[4 * a + 3]);
}

// ---- voxel-grid thinning ---------------------------------------------------------------------------------------------
// voxel of a row: floor(double(v) / leaf) per axis; a coordinate whose voxel index leaves the key range (NaN included)
// skips the row.  There is no sticky error: a localiser must survive a bad point.
__device__ inline bool loc_voxel_key(const float *__restrict__ r, double leaf, uint64_t &key) {
  long long c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double f = floor(__ddiv_rn((double)r[a], leaf));
    if (!(f >= -1048575.0 && f <= 1048575.0)) return false;
    c[a] = (long long)f;
  }
  key = radius_key(c[0], c[1], c[2]);
  return true;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_loc_ds_insert(const float *__restrict__ rows, int64_t ld, int n_max,
                                                               const int *__restrict__ n_dev, double leaf, HashTable h) {
  const int n = min(n_max, max(*n_dev, 0));
  const int p = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  if (p >= n) return;
  uint64_t key;
  if (!loc_voxel_key(rows + (size_t)p * ld, leaf, key)) return;
  const int s = hash_insert(h, key);  // the table holds >= 2 * n_max slots: an insert always finds one
  atomicMin(&h.first[s], p);
}

__device__ inline bool loc_ds_survives(const float *__restrict__ rows, int64_t ld, int p, int n, double leaf, const HashTable &h) {
  if (p >= n) return false;
  uint64_t key;
  if (!loc_voxel_key(rows + (size_t)p * ld, leaf, key)) return false;
  const int s = hash_find_slot(h, key);
  return s >= 0 && h.first[s] == p;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_loc_ds_count(const float *__restrict__ rows, int64_t ld, int n_max,
                                                              const int *__restrict__ n_dev, double leaf, HashTable h,
                                                              int *__restrict__ block_sums) {
  __shared__ int lds[SCAN_BLOCK / 64];
  const int n = min(n_max, max(*n_dev, 0));
  const int p = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  compact_count(loc_ds_survives(rows, ld, p, n, leaf, h), lds, block_sums);
}

// ordered compaction (aux_kernels.inc.h): the survivor of rank k (ascending row index) becomes out[k] = (double)(x, y, z); ranks >= cap are dropped and the
// count saturates at cap
__global__ __launch_bounds__(SCAN_BLOCK) void k_loc_ds_write(const float *__restrict__ rows, int64_t ld, int n_max,
                                                              const int *__restrict__ n_dev, double leaf, HashTable h,
                                                              const int *__restrict__ block_sums, double *__restrict__ out,
                                                              int cap, int *__restrict__ count_out) {
  __shared__ int lds[SCAN_BLOCK / 64];
  __shared__ int wave_off[SCAN_BLOCK / 64];
  const int base = compact_base(block_sums, lds);
  const int n = min(n_max, max(*n_dev, 0));
  const int p = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  const int flag = loc_ds_survives(rows, ld, p, n, leaf, h);
  int kept;
  const int k = compact_rank(base, flag, wave_off, kept);
  if (flag && k < cap) {
    const float *r = rows + (size_t)p * ld;
    double *o = out + (size_t)k * 3;
    o[0] = (double)r[0], o[1] = (double)r[1], o[2] = (double)r[2];
  }
  if (compact_last_thread()) *count_out = min(kept, cap);
}

// ---- alignment -------------------------------------------------------------------------------------------------------
struct LocPose {
  double m[16];
};
constexpr int LOC_TERMS = 29;       // 21 upper-triangle entries of H, 6 of g = sum J^T e, sum d^2, the count
constexpr int LOC_PTS = 32;         // scan points of one workgroup of launch A (one wave per point, 8 rounds of 4)
constexpr int LOC_SEG = 8;          // launch B sums the partial rows as LOC_SEG runs of consecutive blocks

__global__ void k_loc_init(LocPose T, double *__restrict__ T_out, int *__restrict__ status, int *__restrict__ done) {
  const int t = threadIdx.x;
  if (t < 16) T_out[t] = T.m[t];
  if (t < 4) status[t] = t == 0 ? 1 : 0;  // 1 = iterations exhausted, unless an iteration says otherwise
  if (t == 0) *done = 0;
}

// column i of J = [ -[q]x | I ] (the three residual rows)
__device__ inline void loc_jcol(int i, double qx, double qy, double qz, double c[3]) {
  c[0] = c[1] = c[2] = 0.0;
  switch (i) {
    case 0: c[1] = -qz, c[2] = qy; break;
    case 1: c[0] = qz, c[2] = -qx; break;
    case 2: c[0] = -qy, c[1] = qx; break;
    case 3: c[0] = 1.0; break;
    case 4: c[1] = 1.0; break;
    default: c[2] = 1.0; break;
  }
}
__device__ inline double loc_dot3(const double a[3], const double b[3]) {
  return loc_add(loc_add(loc_mul(a[0], b[0]), loc_mul(a[1], b[1])), loc_mul(a[2], b[2]));
}

// The nearest map point of q within d2 <= r2, by a group of W consecutive lanes of a wave (all W lanes call, with the same q
// and r2; lane = the lane's index in its group; W = 64: the whole wave): the lanes look up the 27 cells around q, one or, for
// W < 27, two each, then all W lanes stride over the cells' map points with the exact test d2 = (ex*ex + ey*ey) + ez*ez
// <= r2; the group's minimum is taken over (d2, map index), so ties go to the lowest map index and the result does not
// depend on W.  Every lane gets best = that d2 and best_j = that index; best_j = 0x7FFFFFFF where there is none (q not finite
// or beyond the key range included).  The one definition behind k_loc_assoc and k_loc_match (loc_match_kernels.inc.h).
template <int W>
__device__ inline void loc_nearest(const RadiusGrid &g, const double q[3], double r2, int lane, double &best, int &best_j) {
  static_assert(W == 64 || W == 32 || W == 16, "27 cells in at most two rounds of W lanes");
  constexpr int NC = (27 + W - 1) / W;
  long long cx, cy, cz;
  int c_lo[NC], c_hi[NC];
  const bool in_range = radius_cell(q[0], g.cell_size, cx) && radius_cell(q[1], g.cell_size, cy) && radius_cell(q[2], g.cell_size, cz);
#pragma unroll
  for (int u = 0; u < NC; ++u) {
    const int cell = lane + u * W;
    c_lo[u] = c_hi[u] = 0;
    if (cell < 27 && in_range) {
      const int s = hash_find_slot(g.h, radius_key(cx + (cell % 3 - 1), cy + ((cell / 3) % 3 - 1), cz + (cell / 9 - 1)));
      if (s >= 0) {
        const int c = g.h.rank[s];
        c_lo[u] = g.cell_start[c], c_hi[u] = g.cell_start[c + 1];
      }
    }
  }
  best = INFINITY;
  best_j = 0x7FFFFFFF;
  for (int c = 0; c < 27; ++c) {
    const int u = NC == 1 ? 0 : c / W;
    const int lo = __shfl(NC == 1 ? c_lo[0] : (u ? c_lo[NC - 1] : c_lo[0]), c % W, W);
    const int hi = __shfl(NC == 1 ? c_hi[0] : (u ? c_hi[NC - 1] : c_hi[0]), c % W, W);
    for (int t = lo + lane; t < hi; t += W) {
      const int j = g.cell_pts[t];
      const double ex = q[0] - g.xyz[(size_t)j * 3], ey = q[1] - g.xyz[(size_t)j * 3 + 1], ez = q[2] - g.xyz[(size_t)j * 3 + 2];
      const double d2 = loc_add(loc_add(loc_mul(ex, ex), loc_mul(ey, ey)), loc_mul(ez, ez));
      if (d2 <= r2 && (d2 < best || (d2 == best && j < best_j))) best = d2, best_j = j;
    }
  }
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) {
    const double od = __shfl_xor(best, o, W);
    const int oj = __shfl_xor(best_j, o, W);
    if (od < best || (od == best && oj < best_j)) best = od, best_j = oj;
  }
}

// Launch A.  One wave per scan point: q = R p + t, then loc_nearest within the grid's radius.  Lane l < 29 then forms
// term l of the point, the workgroup adds its LOC_PTS points in point order, and thread l writes entry l of the
// workgroup's partial row.
__global__ __launch_bounds__(256) void k_loc_assoc(const double *__restrict__ pts, const int *__restrict__ n_dev, int cap,
                                                    RadiusGrid g, const double *__restrict__ T, const int *__restrict__ done,
                                                    double *__restrict__ partial) {
  __shared__ double terms[LOC_PTS][LOC_TERMS];
  if (*done) return;
  const int n = min(cap, max(*n_dev, 0));
  const int base = blockIdx.x * LOC_PTS;
  if (base >= n) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double R[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) R[i] = T[i];
  for (int k = wave; k < LOC_PTS; k += 4) {
    const int i = base + k;
    double term = 0.0;
    if (i < n) {
      const double px = pts[(size_t)i * 3], py = pts[(size_t)i * 3 + 1], pz = pts[(size_t)i * 3 + 2];
      double q[3];
      loc_transform(R, px, py, pz, q);
      double best;
      int best_j;
      loc_nearest<64>(g, q, g.r2, lane, best, best_j);
      if (best_j != 0x7FFFFFFF && lane < LOC_TERMS) {
        const int j = best_j;
        const double e[3] = {q[0] - g.xyz[(size_t)j * 3], q[1] - g.xyz[(size_t)j * 3 + 1], q[2] - g.xyz[(size_t)j * 3 + 2]};
        if (lane < 21) {
          int r = 0, l = lane;
          while (l >= 6 - r) l -= 6 - r, ++r;   // upper triangle, row-major: (r, r + l)
          double a[3], b[3];
          loc_jcol(r, q[0], q[1], q[2], a);
          loc_jcol(r + l, q[0], q[1], q[2], b);
          term = loc_dot3(a, b);
        } else if (lane < 27) {
          double a[3];
          loc_jcol(lane - 21, q[0], q[1], q[2], a);
          term = loc_dot3(a, e);
        } else if (lane == 27) {
          term = loc_dot3(e, e);
        } else {
          term = 1.0;
        }
      }
    }
    if (lane < LOC_TERMS) terms[k][lane] = term;
  }
  __syncthreads();
  if (threadIdx.x < LOC_TERMS) {
    double s = 0.0;
    for (int k = 0; k < LOC_PTS; ++k) s = loc_add(s, terms[k][threadIdx.x]);
    partial[(size_t)blockIdx.x * LOC_TERMS + threadIdx.x] = s;
  }
}

// The partial rows of `nb` workgroups added in block order by 256 threads t = 0 .. 255 (every thread of the workgroup must
// call, for the barriers): thread (sg, col) adds the rows of its run of consecutive blocks in order, thread col adds the
// LOC_SEG runs in order.  tot[0 .. LOC_TERMS) holds the sums once the workgroup has passed the barrier at the end.
__device__ inline void loc_sum_rows(const double *__restrict__ partial, int nb, int t, double (*seg)[32], double *tot) {
  const int col = t & 31, sg = t >> 5;
  if (col < LOC_TERMS) {
    const int per = (nb + LOC_SEG - 1) / LOC_SEG;
    const int b1 = min(nb, (sg + 1) * per);
    double s = 0.0;
    for (int b = sg * per; b < b1; ++b) s = loc_add(s, partial[(size_t)b * LOC_TERMS + col]);
    seg[sg][col] = s;
  }
  __syncthreads();
  if (t < LOC_TERMS) {
    double s = 0.0;
    for (int i = 0; i < LOC_SEG; ++i) s = loc_add(s, seg[i][t]);
    tot[t] = s;
  }
  __syncthreads();
}

// One Gauss-Newton step from the summed row tot, by one thread: the normal and trace rows of `iter`, status[1] and
// status[2], the 6 x 6 Cholesky solve, Rodrigues, the pose update.  Returns -1 after a step (vn = |v|, th = |omega|, also in
// the trace row), or the final code 2 (too few correspondences) / 3 (singular) with T = T_init and status[0] = the code.
// What a step means for the call is the caller's: loc_solve_body below, k_ndt_pyr_solve in ndt_pyramid_kernels.inc.h.
//
// The arrays of the 6 x 6 solve live where the caller puts them (loc_solve_step_in): a kernel that may not use scratch memory
// hands in workgroup memory (k_ndt_pyr_solve_batch, ndt_pyramid_batch_kernels.inc.h); loc_solve_step keeps them private.
struct alignas(16) LocSolveWork {
  double L[6][6], H[6][6];
};

__device__ inline int loc_solve_step_in(LocSolveWork &w, const double *tot, int iter, int min_corr,
                                        const double *__restrict__ T_init, double *__restrict__ T, int *__restrict__ status,
                                        double *__restrict__ trace, double *__restrict__ normal, double &vn_out,
                                        double &th_out) {
  const int n_corr = (int)tot[28];
  const double sum_d2 = tot[27];
  double(&L)[6][6] = w.L, (&H)[6][6] = w.H;
  double b[6];
  for (int i = 0; i < 6; ++i) b[i] = -tot[21 + i];
  if (normal) {
    double *o = normal + (size_t)iter * 28;
    for (int i = 0; i < 21; ++i) o[i] = tot[i];
    for (int i = 0; i < 6; ++i) o[21 + i] = b[i];
    o[27] = sum_d2;
  }
  double *tr = trace + (size_t)iter * 4;
  tr[0] = (double)n_corr, tr[1] = sum_d2, tr[2] = 0.0, tr[3] = 0.0;
  status[1] = iter + 1;
  status[2] = n_corr;
  int code = -1;
  double y[6], x[6];
  if (n_corr < min_corr) {
    code = 2;
  } else {
    for (int i = 0, k = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j, ++k) H[i][j] = H[j][i] = tot[k];
    for (int j = 0; j < 6 && code < 0; ++j) {
      double d = H[j][j];
      for (int k = 0; k < j; ++k) d = loc_add(d, -loc_mul(L[j][k], L[j][k]));
      if (!(d > 0.0)) {
        code = 3;
        break;
      }
      const double ljj = __dsqrt_rn(d);
      L[j][j] = ljj;
      for (int i = j + 1; i < 6; ++i) {
        double s = H[i][j];
        for (int k = 0; k < j; ++k) s = loc_add(s, -loc_mul(L[i][k], L[j][k]));
        L[i][j] = __ddiv_rn(s, ljj);
      }
    }
  }
  if (code < 0) {
    for (int i = 0; i < 6; ++i) {
      double s = b[i];
      for (int k = 0; k < i; ++k) s = loc_add(s, -loc_mul(L[i][k], y[k]));
      y[i] = __ddiv_rn(s, L[i][i]);
    }
    for (int i = 5; i >= 0; --i) {
      double s = y[i];
      for (int k = i + 1; k < 6; ++k) s = loc_add(s, -loc_mul(L[k][i], x[k]));
      x[i] = __ddiv_rn(s, L[i][i]);
    }
    bool finite = true;
    for (int i = 0; i < 6; ++i) finite = finite && isfinite(x[i]);
    if (!finite) code = 3;   // an overflowing solve is a singular system too
  }
  if (code >= 0) {
    for (int i = 0; i < 16; ++i) T[i] = T_init[i];
    status[0] = code;
    return code;
  }
  const double wx = x[0], wy = x[1], wz = x[2];
  const double th2 = loc_add(loc_add(loc_mul(wx, wx), loc_mul(wy, wy)), loc_mul(wz, wz));
  const double th = __dsqrt_rn(th2);
  const double vn = __dsqrt_rn(loc_add(loc_add(loc_mul(x[3], x[3]), loc_mul(x[4], x[4])), loc_mul(x[5], x[5])));
  // Exp(w) = I + a K + c K^2, K = [w]x, a = sin(th) / th, c = 2 sin^2(th / 2) / th^2; first order below 1e-12
  double a = 1.0, c = 0.0;
  if (th >= 1e-12) {
    const double sh = sin(loc_mul(0.5, th));
    a = __ddiv_rn(sin(th), th);
    c = __ddiv_rn(loc_mul(2.0, loc_mul(sh, sh)), th2);
  }
  const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  double E[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double k2 = loc_add(loc_add(loc_mul(K[i][0], K[0][j]), loc_mul(K[i][1], K[1][j])), loc_mul(K[i][2], K[2][j]));
      E[i][j] = loc_add(loc_add(i == j ? 1.0 : 0.0, loc_mul(a, K[i][j])), loc_mul(c, k2));
    }
  double Tn[12];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = loc_add(loc_add(loc_mul(E[i][0], T[j]), loc_mul(E[i][1], T[4 + j])), loc_mul(E[i][2], T[8 + j]));
      if (j == 3) s = loc_add(s, x[3 + i]);
      Tn[4 * i + j] = s;
    }
  for (int i = 0; i < 12; ++i) T[i] = Tn[i];
  tr[2] = vn, tr[3] = th;
  vn_out = vn, th_out = th;
  return -1;
}

__device__ inline int loc_solve_step(const double *tot, int iter, int min_corr, const double *__restrict__ T_init,
                                     double *__restrict__ T, int *__restrict__ status, double *__restrict__ trace,
                                     double *__restrict__ normal, double &vn_out, double &th_out) {
  LocSolveWork w;
  return loc_solve_step_in(w, tot, iter, min_corr, T_init, T, status, trace, normal, vn_out, th_out);
}

// Launch B for one pose, by one workgroup of 256 (k_loc_solve; k_loc_solve_batch in ndt_batch_kernels.inc.h runs it once per
// hypothesis): loc_sum_rows, then thread 0 does the rest.  T_init is read only when the status becomes 2 or 3.
__device__ inline void loc_solve_body(const double *__restrict__ partial, const int *__restrict__ n_dev, int cap, int iter,
                                      int min_corr, double tol_t, double tol_r, const double *__restrict__ T_init,
                                      double *__restrict__ T, int *__restrict__ status, int *__restrict__ done,
                                      double *__restrict__ trace, double *__restrict__ normal, double (*seg)[32],
                                      double *tot) {
  if (*done) return;
  const int n = min(cap, max(*n_dev, 0));
  loc_sum_rows(partial, (n + LOC_PTS - 1) / LOC_PTS, threadIdx.x, seg, tot);
  if (threadIdx.x != 0) return;
  double vn, th;
  if (loc_solve_step(tot, iter, min_corr, T_init, T, status, trace, normal, vn, th) >= 0) {
    *done = 1;
    return;
  }
  if (vn < tol_t && th < tol_r) {
    status[0] = 0;
    *done = 1;
  }
}

// Launch B, one workgroup of 256.
__global__ __launch_bounds__(256) void k_loc_solve(const double *__restrict__ partial, const int *__restrict__ n_dev, int cap,
                                                    int iter, int min_corr, double tol_t, double tol_r, LocPose T_init,
                                                    double *__restrict__ T, int *__restrict__ status, int *__restrict__ done,
                                                    double *__restrict__ trace, double *__restrict__ normal) {
  __shared__ double seg[LOC_SEG][32];
  __shared__ double tot[32];
  loc_solve_body(partial, n_dev, cap, iter, min_corr, tol_t, tol_r, T_init.m, T, status, done, trace, normal, seg, tot);
}

#pragma clang fp contract(fast)
