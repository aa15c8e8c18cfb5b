// ndt_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after loc_kernels.inc.h): the NDT
// (point-to-distribution) scan-to-map localiser (host side: ndt_host.inc.h; ABI: the "NDT localiser" section of
// include/sps_hip.h).
//
//   k_ndt_cells   (map build)                 per map cell: n, mean, sample covariance, Jacobi eigen-decomposition, floored
//                                             eigenvalues, inverse covariance -> one 80-byte record (and S for an online map)
//   k_ndt_assoc   (launch A of an iteration)  q = R p + t, the records of q's cell and its face neighbours, the
//                                             normal-equation terms of every contributing cell (its body a template
//                                             over the scan: NdtPoints here, NdtCells of ndt_d2d_kernels.inc.h)
//
// This file also holds the one definition of what the batch, search and update kernels share with these two:
//   ndt_list_moments, ndt_record_from_moments   a cell's moments from its point list; its record from (n, mean, S)
//   ndt_floored_eigen                           the Jacobi sweeps and the eigenvalue floor under every record (also the scan's
//                                               cells of ndt_d2d_kernels.inc.h)
//   ndt_cell_key, ndt_cell_of                   the cell of a point (radius_cell of aux_kernels.inc.h) and its id in the map
//   ndt_cell_hit                                one cell's contribution to one point
//   ndt_assoc_body, ndt_assoc_reduce            launch A: phase 1 over the scan's policy type, phases 2 and 3 from the hits in LDS
// with loc_transform of loc_kernels.inc.h in front.  That the entry points agree bit for bit follows from that.
//
// Launch B is k_loc_solve unchanged: the partial rows have its layout (21 of H, 6 of g, the score, the count; one row per
// LOC_PTS points).  As in loc_kernels.inc.h everything is float64, every operation is rounded on its own (contraction is
// off, products and sums go through loc_mul / loc_add) and no sum depends on the order in which threads arrive.

#pragma clang fp contract(off)

constexpr int NDT_REC = 10;      // doubles of a cell record: mean[3], icov[6] (xx, xy, xz, yy, yz, zz), valid (1.0 / 0.0)
constexpr int NDT_SWEEPS = 8;    // cyclic Jacobi sweeps of the 3 x 3 eigen-decomposition (fixed: no convergence test)
constexpr int NDT_LANES = 8;     // lanes of one scan point in k_ndt_assoc
constexpr int NDT_HIT = 11;      // doubles a contributing cell leaves in LDS: a = -d1 w, icov[6], y = icov x [3], the score
static_assert(LOC_PTS * NDT_LANES == 256, "k_ndt_assoc: one workgroup of 256 covers LOC_PTS points");

struct NdtMap {
  HashTable h;             // cell key -> cell id (rank); keys == nullptr: no map built
  const double *rec;       // [C][NDT_REC]
  const int *count;        // [C] points of the cell
  const uint64_t *keys;    // [C] the cell keys as uploaded (debug getter)
  int n_cells;
  double resolution;
};

struct NdtGauss {
  double nd1, d2;          // -d1 and d2 of the mixture's Gaussian fit (host, float64)
};

// ---- the map -----------------------------------------------------------------------------------------------------------
// One Jacobi rotation that zeroes a[p][q].  t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (aqq - app) / (2 apq).
__device__ inline void ndt_rotate(double a[3][3], double v[3][3], int p, int q) {
  const double apq = a[p][q];
  if (apq == 0.0) return;
  const int r = 3 - p - q;
  const double theta = __ddiv_rn(loc_add(a[q][q], -a[p][p]), loc_mul(2.0, apq));
  const double at = fabs(theta);
  double t = __ddiv_rn(1.0, loc_add(at, __dsqrt_rn(loc_add(loc_mul(theta, theta), 1.0))));
  if (theta < 0.0) t = -t;
  const double c = __ddiv_rn(1.0, __dsqrt_rn(loc_add(loc_mul(t, t), 1.0)));
  const double s = loc_mul(t, c);
  a[p][p] = loc_add(a[p][p], -loc_mul(t, apq));
  a[q][q] = loc_add(a[q][q], loc_mul(t, apq));
  a[p][q] = a[q][p] = 0.0;
  const double arp = a[r][p], arq = a[r][q];
  a[r][p] = a[p][r] = loc_add(loc_mul(c, arp), -loc_mul(s, arq));
  a[r][q] = a[q][r] = loc_add(loc_mul(s, arp), loc_mul(c, arq));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vkp = v[k][p], vkq = v[k][q];
    v[k][p] = loc_add(loc_mul(c, vkp), -loc_mul(s, vkq));
    v[k][q] = loc_add(loc_mul(s, vkp), loc_mul(c, vkq));
  }
}

// n points (list entries [lo, hi) of cell_pts, read in list order: ascending map index) -> their mean and
// S = sum (p - mean)(p - mean)^T as (xx, xy, xz, yy, yz, zz): one pass for the mean, one for the six sums
__device__ inline void ndt_list_moments(const int *__restrict__ cell_pts, const double *__restrict__ xyz, int lo, int hi,
                                        int n_map, int n, double mu[3], double S[6]) {
  double sum[3] = {0.0, 0.0, 0.0};
  for (int t = lo; t < hi; ++t) {
    const int j = cell_pts[t];
    if (j < 0 || j >= n_map) continue;   // a malformed list reads nothing out of bounds
#pragma unroll
    for (int a = 0; a < 3; ++a) sum[a] = loc_add(sum[a], xyz[(size_t)j * 3 + a]);
  }
  for (int a = 0; a < 3; ++a) mu[a] = n > 0 ? __ddiv_rn(sum[a], (double)n) : 0.0;
  for (int i = 0; i < 6; ++i) S[i] = 0.0;
  for (int t = lo; t < hi; ++t) {
    const int j = cell_pts[t];
    if (j < 0 || j >= n_map) continue;
    const double dx = loc_add(xyz[(size_t)j * 3], -mu[0]), dy = loc_add(xyz[(size_t)j * 3 + 1], -mu[1]),
                 dz = loc_add(xyz[(size_t)j * 3 + 2], -mu[2]);
    S[0] = loc_add(S[0], loc_mul(dx, dx)), S[1] = loc_add(S[1], loc_mul(dx, dy)), S[2] = loc_add(S[2], loc_mul(dx, dz));
    S[3] = loc_add(S[3], loc_mul(dy, dy)), S[4] = loc_add(S[4], loc_mul(dy, dz)), S[5] = loc_add(S[5], loc_mul(dz, dz));
  }
}

// The eigen-decomposition that every record is made from, for n >= 2: the sample covariance S / (n - 1), NDT_SWEEPS cyclic
// Jacobi sweeps (eigenvectors: the columns of v), the eigenvalues floored at eig_ratio times the largest.  lmax is the
// largest eigenvalue before the floor.  One definition for the map's records (ndt_record_from_moments below: the inverse
// covariance) and the scan's (ndt_d2d_kernels.inc.h: the covariance itself).
__device__ inline void ndt_floored_eigen(int n, const double S[6], double eig_ratio, double v[3][3], double lam[3], double &lmax) {
  const double nm1 = (double)(n - 1);
  double cv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) cv[i] = __ddiv_rn(S[i], nm1);
  double a[3][3] = {{cv[0], cv[1], cv[2]}, {cv[1], cv[3], cv[4]}, {cv[2], cv[4], cv[5]}};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < NDT_SWEEPS; ++sweep) {
    ndt_rotate(a, v, 0, 1);
    ndt_rotate(a, v, 0, 2);
    ndt_rotate(a, v, 1, 2);
  }
  lam[0] = a[0][0], lam[1] = a[1][1], lam[2] = a[2][2];
  lmax = fmax(fmax(lam[0], lam[1]), lam[2]);
  const double lfloor = loc_mul(eig_ratio, lmax);
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (lam[i] < lfloor) lam[i] = lfloor;
}

// The record of a cell from (n, mean, S): ndt_floored_eigen, inverse covariance, the validity flag.  The map build
// (k_ndt_cells) and the online update (k_ndt_upd_merge, ndt_update_kernels.inc.h) both end here.
__device__ inline void ndt_record_from_moments(int n, const double mu[3], const double S[6], int min_points, double eig_ratio,
                                               double *__restrict__ o) {
  double icov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool valid = n >= min_points && n >= 2;
  if (n >= 2) {
    double v[3][3], lam[3], lmax;
    ndt_floored_eigen(n, S, eig_ratio, v, lam, lmax);
    valid = valid && lmax > 0.0;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j, ++k)
        icov[k] = loc_add(loc_add(__ddiv_rn(loc_mul(v[i][0], v[j][0]), lam[0]), __ddiv_rn(loc_mul(v[i][1], v[j][1]), lam[1])),
                          __ddiv_rn(loc_mul(v[i][2], v[j][2]), lam[2]));
  }
  for (int a = 0; a < 3; ++a) valid = valid && isfinite(mu[a]);
  for (int i = 0; i < 6; ++i) valid = valid && isfinite(icov[i]);
  o[0] = mu[0], o[1] = mu[1], o[2] = mu[2];
#pragma unroll
  for (int i = 0; i < 6; ++i) o[3 + i] = icov[i];
  o[9] = valid ? 1.0 : 0.0;
}

// One thread per cell.  S_out (null: a static map) keeps the cell's S beside the record, for the online update to merge into.
__global__ __launch_bounds__(256) void k_ndt_cells(const int *__restrict__ cell_start, const int *__restrict__ cell_pts,
                                                    const double *__restrict__ xyz, int n_cells, int n_map, int min_points,
                                                    double eig_ratio, double *__restrict__ rec, int *__restrict__ count,
                                                    double *__restrict__ S_out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cells) return;
  const int lo = max(cell_start[c], 0), hi = min(cell_start[c + 1], n_map);
  const int n = max(hi - lo, 0);
  double mu[3], S[6];
  ndt_list_moments(cell_pts, xyz, lo, hi, n_map, n, mu, S);
  if (S_out)
    for (int i = 0; i < 6; ++i) S_out[(size_t)c * 6 + i] = S[i];
  ndt_record_from_moments(n, mu, S, min_points, eig_ratio, rec + (size_t)c * NDT_REC);
  count[c] = n;
}

// debug getter: the records split into the arrays the parity tests compare (any output may be null)
__global__ void k_ndt_cells_get(NdtMap m, unsigned long long *__restrict__ key_out, int *__restrict__ count_out,
                                double *__restrict__ mean_out, double *__restrict__ icov_out, int *__restrict__ valid_out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m.n_cells) return;
  const double *r = m.rec + (size_t)c * NDT_REC;
  if (key_out) key_out[c] = m.keys[c];
  if (count_out) count_out[c] = m.count[c];
  if (mean_out)
    for (int a = 0; a < 3; ++a) mean_out[(size_t)c * 3 + a] = r[a];
  if (icov_out)
    for (int i = 0; i < 6; ++i) icov_out[(size_t)c * 6 + i] = r[3 + i];
  if (valid_out) valid_out[c] = r[9] != 0.0;
}

// ---- alignment -------------------------------------------------------------------------------------------------------
// row i of the symmetric 3 x 3 matrix stored as (xx, xy, xz, yy, yz, zz), times b
__device__ inline double ndt_symrow(const double *m, int i, const double b[3]) {
  const double r[3] = {i == 0 ? m[0] : (i == 1 ? m[1] : m[2]), i == 0 ? m[1] : (i == 1 ? m[3] : m[4]),
                       i == 0 ? m[2] : (i == 1 ? m[4] : m[5])};
  return loc_dot3(r, b);
}

// The key of the cell of q (radius_cell per axis: floor of a true division, the key range) moved to face neighbour `sub`
// (0: q's own cell, then +x, -x, +y, -y, +z, -z); false where q or the neighbour leaves the key range.
__device__ inline bool ndt_cell_key(const double q[3], double res, int sub, uint64_t &key) {
  long long c[3] = {0, 0, 0};
  // all three axes are evaluated (& and not &&), as in the code of the kernels that this one definition replaced
  if (!(radius_cell(q[0], res, c[0]) & radius_cell(q[1], res, c[1]) & radius_cell(q[2], res, c[2]))) return false;
  if (sub > 0) {
    long long &s = c[(sub - 1) >> 1];
    s += (sub & 1) ? 1 : -1;
    if (s < -RADIUS_CELL_MAX || s > RADIUS_CELL_MAX) return false;
  }
  key = radius_key(c[0], c[1], c[2]);
  return true;
}

// the id of that cell in the map, -1 where the map has none
__device__ inline int ndt_cell_of(const NdtMap &m, const double q[3], int sub) {
  uint64_t key;
  if (!ndt_cell_key(q, m.resolution, sub, key)) return -1;
  const int s = hash_find_slot(m.h, key);
  const int cell = s >= 0 ? m.h.rank[s] : -1;
  return cell >= 0 && cell < m.n_cells ? cell : -1;
}

// One cell's contribution to the point q, from the cell's record: x = q - mean, y = icov x, e = exp(-d2 x.y / 2), w = d2 e.
// False where the cell is not valid or w fails the guard; true hands back e, w, y and the record's icov.
__device__ inline bool ndt_cell_hit(const double q[3], const double *__restrict__ rec, const NdtGauss &gs, double &e, double &w,
                                    double y[3], double icov[6]) {
  double r[NDT_REC];   // one contiguous 80-byte record
#pragma unroll
  for (int j = 0; j < NDT_REC; ++j) r[j] = rec[j];
  if (r[9] == 0.0) return false;
  const double x[3] = {loc_add(q[0], -r[0]), loc_add(q[1], -r[1]), loc_add(q[2], -r[2])};
#pragma unroll
  for (int a = 0; a < 3; ++a) y[a] = ndt_symrow(r + 3, a, x);
  e = exp(loc_mul(-0.5, loc_mul(gs.d2, loc_dot3(x, y))));
  w = loc_mul(gs.d2, e);
#pragma unroll
  for (int j = 0; j < 6; ++j) icov[j] = r[3 + j];
  return w >= 0.0 && w <= 1.0;   // NaN fails both: the guard of ndt_omp
}

// Launch A.  NDT_LANES lanes per element of the scan (a point, a source cell), LOC_PTS elements per workgroup.
//   phase 1: lane c < neighbours looks up cell c of the element's place (ndt_cell_of) and, where the cell contributes
//            (Scan::hit), leaves a, the inverse covariance, y and the score in LDS;
//   phase 2: lane l forms terms l, l + 8, l + 16, l + 24 of the element, adding the contributing cells in lookup order;
//   phase 3: thread l < LOC_TERMS adds the workgroup's elements in index order and writes entry l of the partial row.
// The body (ndt_assoc_body below) is shared with k_ndt_assoc_batch (ndt_batch_kernels.inc.h), which runs it once per
// hypothesis, and with the pyramid's launches: T is the pose, partial the rows of that pose, blockIdx.x the workgroup's
// place among them.
struct NdtAssocLds {
  double hit[LOC_PTS][7][NDT_HIT];
  int hit_ok[LOC_PTS][NDT_LANES];
  double terms[LOC_PTS][LOC_TERMS];
};

// Phases 2 and 3 of launch A, from the hits that phase 1 left in LDS (every thread of the workgroup must call, for the
// barriers): k is the thread's element of the workgroup, sub its lane, q the element's place in the map frame.  A source
// cell's hit holds the combined inverse covariance where a point's hit holds the cell's.
__device__ inline void ndt_assoc_reduce(NdtAssocLds &lds, int k, int sub, const double q[3], int neighbours,
                                        double *__restrict__ partial) {
  double(*hit)[7][NDT_HIT] = lds.hit;
  int(*hit_ok)[NDT_LANES] = lds.hit_ok;
  double(*terms)[LOC_TERMS] = lds.terms;
  __syncthreads();
  for (int l = sub; l < LOC_TERMS; l += NDT_LANES) {
    double term = 0.0;
    int any = 0;
    for (int c = 0; c < neighbours; ++c) {
      if (!hit_ok[k][c]) continue;
      any = 1;
      const double *o = hit[k][c];
      double v;
      if (l < 21) {
        int r = 0, cl = l;
        while (cl >= 6 - r) cl -= 6 - r, ++r;   // upper triangle, row-major: (r, r + cl)
        double ja[3], jb[3];
        loc_jcol(r, q[0], q[1], q[2], ja);
        loc_jcol(r + cl, q[0], q[1], q[2], jb);
        const double u[3] = {ndt_symrow(o + 1, 0, jb), ndt_symrow(o + 1, 1, jb), ndt_symrow(o + 1, 2, jb)};
        v = loc_mul(o[0], loc_dot3(ja, u));
      } else if (l < 27) {
        double ja[3];
        loc_jcol(l - 21, q[0], q[1], q[2], ja);
        v = loc_mul(o[0], loc_dot3(ja, o + 7));
      } else {
        v = o[10];
      }
      term = loc_add(term, v);
    }
    if (l == 28) term = any ? 1.0 : 0.0;
    terms[k][l] = term;
  }
  __syncthreads();
  if (threadIdx.x < LOC_TERMS) {
    double s = 0.0;
    for (int p = 0; p < LOC_PTS; ++p) s = loc_add(s, terms[p][threadIdx.x]);
    partial[(size_t)blockIdx.x * LOC_TERMS + threadIdx.x] = s;
  }
}

// ---- the scan as a type ----------------------------------------------------------------------------------------------
// What launch A registers is a policy type: how a lane gets its element and its hit, and, for a pyramid, where a level's
// elements and their count lie and which level follows.  NdtPoints: the thinned points, the same array at every level.
// NdtCells (ndt_d2d_kernels.inc.h): the scan's own cells, a slice per level.
//   ELEM                       doubles of one element
//   valid(el)                  false: the element contributes nothing at any pose and is not counted (apart from hit: the
//                              scorer asks once per element, not once per pose)
//   hit(...)                   of a valid element: q = its place at the pose T, and lane `sub`'s contribution: false where
//                              the cell of q adds nothing; true hands back e, w, y and the inverse covariance B
//   level_elems, level_count   the elements of level l of a pyramid, and where their count is
//   next                       the level after l, < 0 where l is the last
//   last                       the level at which the chain of `next` from level 0 ends
struct NdtPoints {
  static constexpr int ELEM = 3;
  __device__ static bool valid(const double *) { return true; }
  __device__ static bool hit(const NdtMap &m, const NdtGauss &gs, const double *T, const double *p, int sub, int neighbours,
                             double q[3], double &e, double &w, double y[3], double B[6]) {
    loc_transform(T, p[0], p[1], p[2], q);
    const int cell = sub < neighbours ? ndt_cell_of(m, q, sub) : -1;
    return cell >= 0 && ndt_cell_hit(q, m.rec + (size_t)cell * NDT_REC, gs, e, w, y, B);
  }
  __device__ static const double *level_elems(const double *pts, int, int) { return pts; }
  __device__ static const int *level_count(const int *n_dev, int) { return n_dev; }
  __device__ static int next(const int *, int, int l, int n_levels, int) { return l == n_levels - 1 ? -1 : l + 1; }
  __device__ static int last(const int *, int, int n_levels, int) { return n_levels - 1; }
};

template <class Scan>
__device__ inline void ndt_assoc_body(const double *__restrict__ elems, const int *__restrict__ n_dev, int cap, const NdtMap &m,
                                      const NdtGauss &gs, int neighbours, const double *__restrict__ T,
                                      double *__restrict__ partial, NdtAssocLds &lds) {
  const int n = min(cap, max(*n_dev, 0));
  const int base = blockIdx.x * LOC_PTS;
  if (base >= n) return;
  const int k = threadIdx.x / NDT_LANES, sub = threadIdx.x % NDT_LANES;
  const int i = base + k;
  double q[3] = {0.0, 0.0, 0.0};
  int ok = 0;
  if (i < n) {
    double el[Scan::ELEM];
#pragma unroll
    for (int j = 0; j < Scan::ELEM; ++j) el[j] = elems[(size_t)i * Scan::ELEM + j];
    if (Scan::valid(el)) {
      double e, w, y[3], B[6];
      if (Scan::hit(m, gs, T, el, sub, neighbours, q, e, w, y, B)) {
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

// The single alignment's launch A stays a kernel of its own per scan (k_ndt_d2d_assoc: ndt_d2d_kernels.inc.h), launched by
// name from its entry point: the plain submit, 61 launches in 1.0 ms, read 0.2 - 0.4 % slower in two sessions through the
// shared host implementation (profiles/ndt_one_scan).
__global__ __launch_bounds__(256) void k_ndt_assoc(const double *__restrict__ pts, const int *__restrict__ n_dev, int cap,
                                                    NdtMap m, NdtGauss gs, int neighbours, const double *__restrict__ T,
                                                    const int *__restrict__ done, double *__restrict__ partial) {
  __shared__ NdtAssocLds lds;
  if (*done) return;
  ndt_assoc_body<NdtPoints>(pts, n_dev, cap, m, gs, neighbours, T, partial, lds);
}

#pragma clang fp contract(fast)
