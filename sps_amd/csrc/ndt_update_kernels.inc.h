// ndt_update_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after ndt_search_kernels.inc.h):
// the bodies of the online NDT map's update (their __global__ kernels, for the single map and the pyramid alike:
// ndt_online_kernels.inc.h; host side: ndt_online_host.inc.h; ABI: the "NDT localiser, online map" section of
// include/sps_hip.h).  The d2d source build (ndt_d2d_kernels.inc.h) calls some of them too.
//
//   (dynamic build: k_ndt_cells of ndt_kernels.inc.h with its S_out set, S = sum (p - mean)(p - mean)^T beside the record)
//   k_ndt_upd_lookup    (update, 1)      q = R p + t (loc_transform), the cell of q (ndt_cell_key) in the map's hash; misses
//                                        meet in the update's own hash
//   k_ndt_upd_found     (update, 2)      one workgroup: founders ranked by point index, ids up to the capacity, info[0..2]
//   k_ndt_upd_resolve   (update, 3)      every point learns its cell id; admitted founders enter the map's hash; per cell
//                                        the batch count and the lowest point index
//   k_ndt_upd_offsets   (update, 4)      one workgroup: the touched cells in order of their lowest point, list offsets
//   k_ndt_upd_fill      (update, 5)      the cells' index lists (any order inside a cell)
//   k_ndt_upd_stats     (update, 6)      one wave per touched cell: indices into ascending order, n_b, mean_b, S_b
//   k_ndt_upd_merge     (update, 7)      one thread per touched cell: forgetting, merge, ndt_record_from_moments
//
// The rules of ndt_kernels.inc.h hold: float64, contraction off, loc_mul / loc_add / __ddiv_rn, no float atomics.  The integer
// atomics are a compare-and-swap on a key, atomicMin of a point index and atomicAdd of a count: none of their results
// depends on the order of arrival.  The one place where arrival order shows, the position of an index inside its cell's
// list after k_ndt_upd_fill, is removed again by k_ndt_upd_stats before any float is added.

#pragma clang fp contract(off)

constexpr int NDT_UPD_MAX_POINTS = 65536;        // SPS_NDT_UPDATE_MAX_POINTS: the single-workgroup scans and the wave's bitmap
constexpr int NDT_UPD_NONE = 0x7F7F7F7F;         // "no point yet" of the atomicMin arrays (the byte 0x7F, memset)
constexpr int NDT_UPD_BLOCK = 1024;              // threads of the two single-workgroup kernels

struct NdtDyn {
  int capacity;            // 0: the map of this context is static
  int min_points;
  double eig_ratio;
  double *rec;             // the arrays of NdtMap, writable.  Invariant kept by every writer (ndt_record_from_moments: valid
  int *count;              // needs n >= 2; the carve's clear zeroes record and count together): rec valid => count >= 2, so
                           // a reader that skips records that are not valid (k_ndt_carve_rays) also skips count = 0
  uint64_t *keys;
  double *S;               // [capacity][6] sum (p - mean)(p - mean)^T (xx, xy, xz, yy, yz, zz)
  int *bcnt;               // [capacity] points of the cell in the running update (0 between updates)
  int *lead;               // [capacity] lowest point index of the cell in the running update (NDT_UPD_NONE between updates)
  int *cstart;             // [capacity] offset of the cell's list in the running update
  int *state;              // [0] cells assigned, [1] cells dropped for capacity since the build
  int *pass;               // [capacity] carving (ndt_carve_kernels.inc.h): rays through the cell's Gaussian, last open carve
  int *hit;                // [capacity] carving: rays that ended in the cell, last open carve
  int *miss;               // [capacity] carving: consecutive carves in which the cell was seen through
};

// the caller's scratch for one update of at most `cap` points
struct NdtUpdScratch {
  double *q;               // [cap][3] map-frame points
  double *bstat;           // [cap][10] per touched cell: n_b, mean_b[3], S_b[6]
  int *cell_of;            // [cap] cell id of the point, -1: skipped or dropped
  int *slot_of;            // [cap] slot in the update's hash where the map's hash missed, else -1
  int *list;               // [cap] point indices grouped by cell
  int *tcell;              // [cap] touched cells
  int *n_touched;          // [1]
  HashTable h;             // keys, first (lowest point index of the key), rank (the founder's cell id, -1: not admitted)
};

__device__ inline bool ndt_upd_gate_open(const int *__restrict__ gate) { return !gate || (unsigned)*gate <= 1u; }

// ---- the update ----------------------------------------------------------------------------------------------------------
// exclusive prefix of v over the NDT_UPD_BLOCK threads of the workgroup (every thread must call); lds: NDT_UPD_BLOCK / 64 ints
__device__ inline int ndt_upd_scan(int v, int *lds, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  int off = 0, tot = 0;
  for (int i = 0; i < NDT_UPD_BLOCK / 64; ++i) {
    const int c = lds[i];
    if (i < wave) off += c;
    tot += c;
  }
  __syncthreads();
  total = tot;
  return off + inc - v;
}

// The bodies of the seven kernels.  A kernel of ndt_online_kernels.inc.h passes a level's map, state, scratch slice and info
// words.  Every body indexes by blockIdx.x / gridDim.x only; blockIdx.y is the caller's.

// 1: one thread per point.  store_q: q goes to s.q (it does not depend on the map: of several levels that share s.q one stores)
__device__ inline void ndt_upd_lookup_body(const double *__restrict__ pts, const int *__restrict__ n_dev, int cap,
                                           const LocPose &Th, const double *__restrict__ T_dev, const int *__restrict__ gate,
                                           const NdtMap &m, const NdtUpdScratch &s, bool store_q) {
  if (!ndt_upd_gate_open(gate)) return;
  const int n = min(cap, max(*n_dev, 0));
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double px = pts[(size_t)i * 3], py = pts[(size_t)i * 3 + 1], pz = pts[(size_t)i * 3 + 2];
  double q[3];
  if (T_dev) loc_transform(T_dev, px, py, pz, q);   // one uniform branch, not a choice of address per entry of the pose
  else loc_transform(Th.m, px, py, pz, q);
  if (store_q) {
#pragma unroll
    for (int a = 0; a < 3; ++a) s.q[(size_t)i * 3 + a] = q[a];
  }
  int cell = -1, slot = -1;
  uint64_t key;
  if (ndt_cell_key(q, m.resolution, 0, key)) {
    const int ms = hash_find_slot(m.h, key);
    if (ms >= 0) {
      cell = m.h.rank[ms];
      if (cell < 0 || cell >= m.n_cells) cell = -1;
    } else {
      slot = hash_insert(s.h, key);   // >= 2 * cap slots: an insert always finds one
      atomicMin(&s.h.first[slot], i);
    }
  }
  s.cell_of[i] = cell;
  s.slot_of[i] = slot;
}

// 2: one workgroup.  A founder is the lowest point index of a missed key; founder r (ascending index) gets the cell id
// assigned + r while that is below the capacity.  Writes info[0..2], the cell counter and the dropped total.
__device__ inline void ndt_upd_found_body(const int *__restrict__ n_dev, int cap, const int *__restrict__ gate, const NdtDyn &d,
                                          const NdtUpdScratch &s, int *__restrict__ info, int *lds) {
  const int n0 = min(max(d.state[0], 0), d.capacity);
  if (!ndt_upd_gate_open(gate)) {
    if (threadIdx.x < 4) info[threadIdx.x] = threadIdx.x == 0 ? n0 : 0;
    return;
  }
  const int n = min(cap, max(*n_dev, 0));
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += NDT_UPD_BLOCK) {
    const int i = i0 + (int)threadIdx.x;
    const int slot = i < n ? s.slot_of[i] : -1;
    const int flag = slot >= 0 && s.h.first[slot] == i;
    int tot;
    const int r = base + ndt_upd_scan(flag, lds, tot);
    if (flag) s.h.rank[slot] = r < d.capacity - n0 ? n0 + r : -1;
    base += tot;
  }
  __syncthreads();   // every thread has read state[0]
  if (threadIdx.x == 0) {
    const int founded = min(base, d.capacity - n0);
    d.state[0] = n0 + founded;
    d.state[1] += base - founded;
    info[0] = n0 + founded, info[1] = founded, info[2] = base - founded;
  }
}

// 3: one thread per point
__device__ inline void ndt_upd_resolve_body(const int *__restrict__ n_dev, int cap, const int *__restrict__ gate,
                                            const NdtMap &m, const NdtDyn &d, const NdtUpdScratch &s) {
  if (!ndt_upd_gate_open(gate)) return;
  const int n = min(cap, max(*n_dev, 0));
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int cell = s.cell_of[i];
  const int slot = s.slot_of[i];
  if (slot >= 0) {
    cell = s.h.rank[slot];
    if (cell >= d.capacity) cell = -1;
    if (cell >= 0 && s.h.first[slot] == i) {   // the admitted founder: at most `capacity` keys ever enter, the load stays <= 0.5
      const uint64_t key = s.h.keys[slot];
      const int ms = hash_insert(m.h, key);
      m.h.rank[ms] = cell;
      d.keys[cell] = key;
    }
    s.cell_of[i] = cell;
  }
  if (cell >= 0) {
    atomicAdd(&d.bcnt[cell], 1);
    atomicMin(&d.lead[cell], i);
  }
}

// 4: one workgroup.  The touched cells in ascending order of their lowest point, the offsets of their lists, info[3].
__device__ inline void ndt_upd_offsets_body(const int *__restrict__ n_dev, int cap, const int *__restrict__ gate, const NdtDyn &d,
                                            const NdtUpdScratch &s, int *__restrict__ info, int *lds) {
  if (!ndt_upd_gate_open(gate)) {
    if (threadIdx.x == 0) *s.n_touched = 0;
    return;
  }
  const int n = min(cap, max(*n_dev, 0));
  int base = 0, nt = 0;
  for (int i0 = 0; i0 < n; i0 += NDT_UPD_BLOCK) {
    const int i = i0 + (int)threadIdx.x;
    const int cell = i < n ? s.cell_of[i] : -1;
    const int flag = cell >= 0 && d.lead[cell] == i;
    const int v = flag ? d.bcnt[cell] : 0;
    int totv, totf;
    const int exv = ndt_upd_scan(v, lds, totv);
    const int exf = ndt_upd_scan(flag, lds, totf);
    if (flag) {
      d.cstart[cell] = base + exv;
      d.bcnt[cell] = 0;   // the cursor of k_ndt_upd_fill, which counts it up to n_b again
      s.tcell[nt + exf] = cell;
    }
    base += totv, nt += totf;
  }
  if (threadIdx.x == 0) {
    *s.n_touched = nt;
    info[3] = base;
  }
}

// 5: one thread per point
__device__ inline void ndt_upd_fill_body(const int *__restrict__ n_dev, int cap, const int *__restrict__ gate, const NdtDyn &d,
                                         const NdtUpdScratch &s) {
  if (!ndt_upd_gate_open(gate)) return;
  const int n = min(cap, max(*n_dev, 0));
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int cell = s.cell_of[i];
  if (cell < 0) return;
  const int pos = d.cstart[cell] + atomicAdd(&d.bcnt[cell], 1);
  if (pos >= 0 && pos < cap) s.list[pos] = i;
}

// lane l's point of a chunk of m <= 64 entries of the ordered list that starts at entry `at` (zeros for l >= m)
__device__ inline void ndt_upd_chunk_point(const NdtUpdScratch &s, int at, int m, int n, double &x, double &y, double &z) {
  x = y = z = 0.0;
  if ((int)threadIdx.x < m) {
    const int j = min(max(s.list[at + (int)threadIdx.x], 0), n - 1);
    x = s.q[(size_t)j * 3], y = s.q[(size_t)j * 3 + 1], z = s.q[(size_t)j * 3 + 2];
  }
}

// 6: one wave (a workgroup of 64) per touched cell.  The cell's indices are distinct values below n, so a bitmap of n bits
// in LDS orders them: set the bits (an integer atomicOr), count the words' bits, write the indices back in ascending order.
// Then the sums of k_ndt_cells over that order: 64 points at a time, lane l holds point l of the chunk and every lane adds
// the chunk's points in order (the same value on every lane).  Linear in n_b + n / 32 whatever the points' spread.
__device__ inline void ndt_upd_stats_body(const int *__restrict__ n_dev, int cap, const int *__restrict__ gate, const NdtDyn &d,
                                          const NdtUpdScratch &s, unsigned *bits) {
  if (!ndt_upd_gate_open(gate)) return;
  const int n = min(min(cap, max(*n_dev, 0)), NDT_UPD_MAX_POINTS);
  const int lane = threadIdx.x;
  const int nt = min(max(*s.n_touched, 0), n);
  for (int t = blockIdx.x; t < nt; t += gridDim.x) {
    const int cell = s.tcell[t];
    const int nb = d.bcnt[cell], st = d.cstart[cell];
    if (nb <= 0 || st < 0 || (long long)st + nb > n) continue;   // never true for lists built above; reads stay in bounds
    const int w0 = max(d.lead[cell], 0) / 32, w1 = (n + 31) / 32;
    for (int w = w0 + lane; w < w1; w += 64) bits[w] = 0u;
    __syncthreads();
    for (int k = lane; k < nb; k += 64) {
      const int j = s.list[st + k];
      if (j >= w0 * 32 && j < n) atomicOr(&bits[j >> 5], 1u << (j & 31));
    }
    __syncthreads();
    int done = 0;
    for (int wb = w0; wb < w1; wb += 64) {
      unsigned w = wb + lane < w1 ? bits[wb + lane] : 0u;
      const int pc = __popc(w);
      int inc = pc;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
      }
      int pos = done + inc - pc;
      while (w) {
        const int b = __ffs((int)w) - 1;
        if (pos < nb) s.list[st + pos] = (wb + lane) * 32 + b;
        ++pos;
        w &= w - 1u;
      }
      done += __shfl(inc, 63, 64);
    }
    __syncthreads();   // the ordered list is visible to the whole wave
    double sum[3] = {0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < nb; k0 += 64) {
      const int m = min(64, nb - k0);
      double x, y, z;
      ndt_upd_chunk_point(s, st + k0, m, n, x, y, z);
      for (int l = 0; l < m; ++l) {
        sum[0] = loc_add(sum[0], __shfl(x, l, 64));
        sum[1] = loc_add(sum[1], __shfl(y, l, 64));
        sum[2] = loc_add(sum[2], __shfl(z, l, 64));
      }
    }
    double mu[3];
    for (int a = 0; a < 3; ++a) mu[a] = __ddiv_rn(sum[a], (double)nb);
    double cv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < nb; k0 += 64) {
      const int m = min(64, nb - k0);
      double x, y, z;
      ndt_upd_chunk_point(s, st + k0, m, n, x, y, z);
      for (int l = 0; l < m; ++l) {
        const double dx = loc_add(__shfl(x, l, 64), -mu[0]), dy = loc_add(__shfl(y, l, 64), -mu[1]),
                     dz = loc_add(__shfl(z, l, 64), -mu[2]);
        cv[0] = loc_add(cv[0], loc_mul(dx, dx)), cv[1] = loc_add(cv[1], loc_mul(dx, dy)), cv[2] = loc_add(cv[2], loc_mul(dx, dz));
        cv[3] = loc_add(cv[3], loc_mul(dy, dy)), cv[4] = loc_add(cv[4], loc_mul(dy, dz)), cv[5] = loc_add(cv[5], loc_mul(dz, dz));
      }
    }
    if (lane == 0) {
      double *o = s.bstat + (size_t)t * 10;
      o[0] = (double)nb, o[1] = mu[0], o[2] = mu[1], o[3] = mu[2];
      for (int i = 0; i < 6; ++i) o[4 + i] = cv[i];
    }
    __syncthreads();   // the bitmap is cleared for the next cell only after every lane has read it
  }
}

// 7: one thread per touched cell: forgetting, merge, the record; the cell's update counters go back to their rest values.
__device__ inline void ndt_upd_merge_body(const int *__restrict__ n_dev, int cap, const int *__restrict__ gate,
                                          int max_cell_points, const NdtDyn &d, const NdtUpdScratch &s) {
  if (!ndt_upd_gate_open(gate)) return;
  const int nt = min(max(*s.n_touched, 0), min(cap, max(*n_dev, 0)));
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const int cell = s.tcell[t];
  const double *b = s.bstat + (size_t)t * 10;
  const int nb = d.bcnt[cell];
  d.bcnt[cell] = 0;
  d.lead[cell] = NDT_UPD_NONE;
  if (nb <= 0) return;
  int n = d.count[cell];
  double mu[3], S[6];
  double *rec = d.rec + (size_t)cell * NDT_REC, *Sg = d.S + (size_t)cell * 6;
  for (int a = 0; a < 3; ++a) mu[a] = rec[a];
  for (int i = 0; i < 6; ++i) S[i] = Sg[i];
  if (max_cell_points >= 2 && n > max_cell_points) {
    const double f = __ddiv_rn((double)(max_cell_points - 1), (double)(n - 1));
    for (int i = 0; i < 6; ++i) S[i] = loc_mul(S[i], f);
    n = max_cell_points;
  }
  int n2;
  if (n <= 0) {
    n2 = nb;
    for (int a = 0; a < 3; ++a) mu[a] = b[1 + a];
    for (int i = 0; i < 6; ++i) S[i] = b[4 + i];
  } else {
    n2 = (int)min((long long)n + nb, 2147483647ll);
    const double dl[3] = {loc_add(b[1], -mu[0]), loc_add(b[2], -mu[1]), loc_add(b[3], -mu[2])};
    const double f = __ddiv_rn((double)nb, (double)n2);
    const double g = __ddiv_rn(loc_mul((double)n, (double)nb), (double)n2);
    for (int a = 0; a < 3; ++a) mu[a] = loc_add(mu[a], loc_mul(dl[a], f));
    int k = 0;
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j, ++k) S[k] = loc_add(loc_add(S[k], b[4 + k]), loc_mul(loc_mul(dl[i], dl[j]), g));
  }
  for (int i = 0; i < 6; ++i) Sg[i] = S[i];
  ndt_record_from_moments(n2, mu, S, d.min_points, d.eig_ratio, rec);
  d.count[cell] = n2;
}

#pragma clang fp contract(fast)
