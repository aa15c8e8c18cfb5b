// ndt_carve_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after ndt_update_kernels.inc.h):
// the bodies of the free-space carving of the online NDT map (their __global__ kernels, for the single map and the pyramid
// alike: ndt_online_kernels.inc.h; host side: ndt_online_host.inc.h; ABI: the "NDT localiser, online map: free-space
// carving" section of include/sps_hip.h).
//
//   k_ndt_carve_begin    (carve, 1)     the gate; pass = hit = 0 for every cell of the capacity, info = 0
//   k_ndt_carve_rays     (carve, 2)     one ray per lane: the end's cell gets a hit, then the cells between the sensor and the
//                                       end margin are walked (Amanatides-Woo in the ray parameter) and every valid Gaussian
//                                       the ray comes within through_sigma of gets a pass
//   k_ndt_carve_decide   (carve, 3)     one thread per assigned cell: miss from (hit, pass), the clear at miss_frames
//
// The rules of ndt_kernels.inc.h hold: float64, contraction off, loc_mul / loc_add / __ddiv_rn, no float atomics.  The only
// atomics are integer atomicAdd of 1 on a cell's pass or hit and of a wave's count on an info word; every float is compared,
// never accumulated across rays, so the outcome depends on the set of rays and the pose only.

#pragma clang fp contract(off)

struct NdtCarveParams {
  double end_margin, sigma2;   // sigma2 = through_sigma * through_sigma (host, float64)
  int min_pass, miss_frames, max_steps;
};

// the lanes of the wave for which `flag` holds, added to *word by lane 0 (all 64 lanes of the wave must call)
__device__ inline void ndt_carve_count(int flag, int *word) {
  const unsigned long long b = __ballot(flag);
  if (b && (threadIdx.x & 63) == 0) atomicAdd(word, __popcll(b));
}

// The bodies of the three kernels (ndt_online_kernels.inc.h).  Every body indexes by blockIdx.x only; blockIdx.y is the
// caller's.

// 1: one thread per cell of the capacity
__device__ inline void ndt_carve_begin_body(const int *__restrict__ gate, const NdtDyn &d, int *__restrict__ info) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < 4) info[c] = 0;
  if (!ndt_upd_gate_open(gate) || c >= d.capacity) return;
  d.pass[c] = 0;
  d.hit[c] = 0;
}

// Does the ray o + s d come within the gate of the cell's Gaussian for some s in [s_in, s_out]?  The point of the line
// closest to the mean in the Gaussian's own metric is s* = d^T A (mu - o) / d^T A d; the segment's closest point is s*
// clamped.  y = A d is formed once and serves both dot products (A is symmetric).
__device__ inline bool ndt_carve_passes(const double *__restrict__ rec, const double o[3], const double d[3], double s_in,
                                        double s_out, double sigma2) {
  double r[NDT_REC];   // one contiguous 80-byte record
#pragma unroll
  for (int j = 0; j < NDT_REC; ++j) r[j] = rec[j];
  if (r[9] == 0.0) return false;   // a valid record has count >= 2: the clear zeroes the record with the count
  const double y[3] = {ndt_symrow(r + 3, 0, d), ndt_symrow(r + 3, 1, d), ndt_symrow(r + 3, 2, d)};
  const double a = loc_dot3(d, y);
  const double w[3] = {loc_add(r[0], -o[0]), loc_add(r[1], -o[1]), loc_add(r[2], -o[2])};
  const double b = loc_dot3(y, w);
  double s = __ddiv_rn(b, a);
  if (!(a > 0.0) || s != s) return false;
  s = fmin(fmax(s, s_in), s_out);
  const double x[3] = {loc_add(loc_add(o[0], loc_mul(s, d[0])), -r[0]), loc_add(loc_add(o[1], loc_mul(s, d[1])), -r[1]),
                       loc_add(loc_add(o[2], loc_mul(s, d[2])), -r[2])};
  const double z[3] = {ndt_symrow(r + 3, 0, x), ndt_symrow(r + 3, 1, x), ndt_symrow(r + 3, 2, x)};
  return loc_dot3(x, z) <= sigma2;
}

// 2: one ray per lane.  Lanes whose ray is over wait for the longest ray of their wave.
__device__ inline void ndt_carve_rays_body(const double *__restrict__ pts, const int *__restrict__ n_dev, int cap,
                                           const LocPose &Th, const double *__restrict__ T_dev, const int *__restrict__ gate,
                                           const NdtMap &m, const NdtDyn &dy, const NdtCarveParams &p, int *__restrict__ info) {
  if (!ndt_upd_gate_open(gate)) return;
  const int n = min(cap, max(*n_dev, 0));
  const int i = blockIdx.x * 256 + threadIdx.x;
  int cast = 0, cut = 0;
  if (i < n) {
    const double px = pts[(size_t)i * 3], py = pts[(size_t)i * 3 + 1], pz = pts[(size_t)i * 3 + 2];
    double o[3], q[3];
    if (T_dev) {   // one uniform branch, not a choice of address per entry of the pose
      o[0] = T_dev[3], o[1] = T_dev[7], o[2] = T_dev[11];
      loc_transform(T_dev, px, py, pz, q);
    } else {
      o[0] = Th.m[3], o[1] = Th.m[7], o[2] = Th.m[11];
      loc_transform(Th.m, px, py, pz, q);
    }
    uint64_t kq, ko;
    const bool finite = isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) && isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]);
    if (finite && ndt_cell_key(q, m.resolution, 0, kq) && ndt_cell_key(o, m.resolution, 0, ko)) {
      cast = 1;
      const int sq = hash_find_slot(m.h, kq);
      const int cq = sq >= 0 ? m.h.rank[sq] : -1;
      if (cq >= 0 && cq < m.n_cells) atomicAdd(&dy.hit[cq], 1);
      const double d[3] = {loc_add(q[0], -o[0]), loc_add(q[1], -o[1]), loc_add(q[2], -o[2])};
      const double L = __dsqrt_rn(loc_dot3(d, d));
      if (!(L <= p.end_margin)) {
        const double s_end = loc_add(1.0, -__ddiv_rn(p.end_margin, L));
        long long c[3];
        int step[3];
        double tmax[3], tdelta[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          c[a] = (long long)((ko >> (21 * a)) & 0x1FFFFFull) - 1048576;   // radius_key's packing, undone
          step[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
          tmax[a] = tdelta[a] = INFINITY;
          if (step[a]) {
            tmax[a] = __ddiv_rn(loc_add(loc_mul((double)(c[a] + (step[a] > 0)), m.resolution), -o[a]), d[a]);
            tdelta[a] = __ddiv_rn(m.resolution, fabs(d[a]));
          }
        }
        double s_in = 0.0;
        for (int done = 1;; ++done) {
          const int ax = tmax[0] <= tmax[1] ? (tmax[0] <= tmax[2] ? 0 : 2) : (tmax[1] <= tmax[2] ? 1 : 2);
          const double t = ax == 0 ? tmax[0] : (ax == 1 ? tmax[1] : tmax[2]);
          const int s = hash_find_slot(m.h, radius_key(c[0], c[1], c[2]));
          if (s >= 0) {
            const int cell = m.h.rank[s];
            if (cell >= 0 && cell < m.n_cells &&
                ndt_carve_passes(m.rec + (size_t)cell * NDT_REC, o, d, s_in, fmin(t, s_end), p.sigma2))
              atomicAdd(&dy.pass[cell], 1);
          }
          if (t >= s_end) break;
          if (done >= p.max_steps) {
            cut = 1;
            break;
          }
          // select by value, not by address: the three arrays stay in registers
          long long cn = 0;
#pragma unroll
          for (int a = 0; a < 3; ++a)
            if (a == ax) {
              c[a] += step[a];
              cn = c[a];
              tmax[a] = loc_add(t, tdelta[a]);
            }
          if (cn < -RADIUS_CELL_MAX || cn > RADIUS_CELL_MAX) break;
          s_in = t;
        }
      }
    }
  }
  ndt_carve_count(cast, &info[0]);
  ndt_carve_count(cut, &info[3]);
}

// 3: one thread per cell of the capacity; the cells below the assigned count decide
__device__ inline void ndt_carve_decide_body(const int *__restrict__ gate, const NdtDyn &d, const NdtCarveParams &p,
                                             int *__restrict__ info) {
  if (!ndt_upd_gate_open(gate)) return;
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int assigned = min(max(d.state[0], 0), d.capacity);
  int seen = 0, cleared = 0;
  if (c < assigned) {
    double *rec = d.rec + (size_t)c * NDT_REC;
    if (d.count[c] > 0 && rec[9] != 0.0) {
      int miss = d.miss[c];
      if (d.hit[c] >= 1) miss = 0;
      else if (d.pass[c] >= p.min_pass) ++miss, seen = 1;
      if (miss >= p.miss_frames) {   // the cell keeps its key, its hash entry and its id
        cleared = 1;
        miss = 0;
        d.count[c] = 0;
        for (int i = 0; i < 6; ++i) d.S[(size_t)c * 6 + i] = 0.0;
        for (int j = 0; j < NDT_REC; ++j) rec[j] = 0.0;
      }
      d.miss[c] = miss;
    }
  }
  ndt_carve_count(seen, &info[1]);
  ndt_carve_count(cleared, &info[2]);
}

#pragma clang fp contract(fast)
