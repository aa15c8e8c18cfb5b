// bbs_kernels.inc.h -- part of sps_hip.hip (included inside its anonymous namespace, after ndt_search_kernels.inc.h): the
// global search, a branch and bound over (x, y, yaw) on a pyramid of 2-D occupancy grids (host side: bbs_host.inc.h; ABI:
// the "NDT localiser, global search" section of include/sps_hip.h).
//
//   k_bbs_pad / k_bbs_pool   the build: G0 into the padded storage of level 0, level l from level l - 1
//   k_bbs_offsets            once per call: the integer cell offsets (dx, dy) of every slice point at every yaw
//   k_bbs_score              per level, the hot path: score[c] = the sum over the points of G_l(i + dx, j + dy), and the
//                            histogram of the scores
//   k_bbs_threshold          per level, one workgroup: the cut "score >= min_score, then the F first" from the histogram
//   k_bbs_count / k_bbs_write  per level: the ordered compaction of the kept nodes (compact_count / compact_base /
//                            compact_rank, aux_kernels.inc.h); the write launch emits the children, at level 0 the leaves
//   k_bbs_top                one workgroup: the K best leaves by (score descending, id ascending), their poses
//
// Scores are int32 sums of bytes that are 0 or 1: exact and independent of any order.  The only atomics are integer adds
// (the histogram and the count of slice points).  A node is its canonical id (a * H + j) * W + i, -1 for a void slot: the
// candidates of a level below L are four slots per kept parent, in the parents' order, and a child outside the grid leaves
// its slot void -- never scored, counted or kept -- so the order of the candidates is that of the list without voids.
// Floating point (k_bbs_offsets and k_bbs_top only) is float64 with every operation rounded on its own.

#pragma clang fp contract(off)

constexpr int BBS_MAX_LEVELS = 8;               // levels 0 .. L with L <= 7 (SPS_BBS_MAX_LEVELS)
constexpr int BBS_MAX_STORE = 16384;            // W + 2^L - 1 and H + 2^L - 1 stay within this: an offset fits 16 bits
constexpr int BBS_MAX_POINTS = 65536;           // scores lie in [0, 65536]
constexpr int BBS_HIST = BBS_MAX_POINTS + 1;
constexpr int BBS_VOID = (int)0x80008000u;      // the packed offset (-32768, -32768): reaches no stored cell from any node
constexpr int BBS_NODES = 64;                   // nodes of one workgroup of k_bbs_score: one per lane, the 4 waves split the points
constexpr int BBS_CHUNK = 1024;                 // offsets of one yaw held in LDS at a time
constexpr int BBS_INFO = 4 + 2 * BBS_MAX_LEVELS;   // info words (SPS_BBS_INFO_WORDS)
// the control words in the scratch: the slots of the candidate list of a level (two words, written by one level's write
// launch and read by the launches of the next), the cut of the current level (keep score > GT,
// and the first QUOTA nodes with score == TIE), the certificate's two accumulators
enum { BBS_C_SLOTS = 0, BBS_C_SLOTS_B, BBS_C_GT, BBS_C_TIE, BBS_C_QUOTA, BBS_C_BOUND, BBS_C_DROPPED, BBS_C_WORDS = 16 };

struct BbsGrid {
  const unsigned char *g;   // (L + 1) levels of Hs rows of Ws bytes; cell (x, y) of any level at [(y + pad) * Ws + x + pad]
  int W, H, Ws, Hs, pad, L;
};

// ---- build ---------------------------------------------------------------------------------------------------------------
__global__ void k_bbs_pad(const unsigned char *__restrict__ g0, BbsGrid b, unsigned char *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)b.Ws * b.Hs) return;
  const int x = (int)(t % b.Ws) - b.pad, y = (int)(t / b.Ws) - b.pad;
  out[t] = (x >= 0 && y >= 0 && g0[(size_t)y * b.W + x]) ? 1 : 0;
}

// level l from level l - 1: G_l(x, y) = max of G_(l-1) at (x, y), (x + h, y), (x, y + h), (x + h, y + h), h = 2^(l-1); a
// read outside the storage is 0
__global__ void k_bbs_pool(BbsGrid b, int l, const unsigned char *__restrict__ below, unsigned char *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)b.Ws * b.Hs) return;
  const int xs = (int)(t % b.Ws), ys = (int)(t / b.Ws), h = 1 << (l - 1);
  int v = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int x = xs + (c & 1) * h, y = ys + (c >> 1) * h;
    if (x < b.Ws && y < b.Hs) v |= below[(size_t)y * b.Ws + x];
  }
  out[t] = (unsigned char)v;
}

// ---- once per call -------------------------------------------------------------------------------------------------------
// floor(w / r) as an integer, false where the quotient is not finite or beyond 2^20 in magnitude
__device__ inline bool bbs_cell(double w, double r, int &out) {
  const double f = __ddiv_rn(w, r);
  if (!(fabs(f) <= 1048576.0)) return false;
  out = (int)floor(f);
  return true;
}

// grid (point blocks, yaws).  offs[a][p] for p < n; rows past n are never written and never read.  Thread 0 of the grid
// also starts the certificate's accumulators (bound -1, nothing dropped).  A point outside the
// slice, or without a cell at this yaw, or whose offset no node can bring onto the storage, is BBS_VOID.
__global__ __launch_bounds__(256) void k_bbs_offsets(const double *__restrict__ pts, const int *__restrict__ n_dev, int cap,
                                                      LocPose T_up, double z_lo, double z_hi, double r,
                                                      const double *__restrict__ yaw_cs, int *__restrict__ offs,
                                                      int *__restrict__ n_slice, int *__restrict__ ctl) {
  const int n = min(cap, max(*n_dev, 0));
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ctl[BBS_C_BOUND] = -1, ctl[BBS_C_DROPPED] = 0;
  if ((int)blockIdx.x * 256 >= n) return;
  int in_slice = 0, word = BBS_VOID;
  if (p < n) {
    double q[3];
    loc_transform(T_up.m, pts[(size_t)p * 3], pts[(size_t)p * 3 + 1], pts[(size_t)p * 3 + 2], q);
    in_slice = q[2] >= z_lo && q[2] <= z_hi;               // NaN fails
    if (in_slice) {
      const double c = yaw_cs[2 * blockIdx.y], s = yaw_cs[2 * blockIdx.y + 1];
      const double u = loc_add(loc_mul(c, q[0]), -loc_mul(s, q[1]));
      const double v = loc_add(loc_mul(s, q[0]), loc_mul(c, q[1]));
      int dx, dy;
      if (bbs_cell(u, r, dx) && bbs_cell(v, r, dy) && abs(dx) < BBS_MAX_STORE && abs(dy) < BBS_MAX_STORE)
        word = (int)(((unsigned)dy << 16) | ((unsigned)dx & 0xFFFFu));
    }
    offs[(size_t)blockIdx.y * cap + p] = word;
  }
  if (blockIdx.y == 0) {
    const unsigned long long bal = __ballot(in_slice);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(n_slice, __popcll(bal));
  }
}

// ---- per level -----------------------------------------------------------------------------------------------------------
struct BbsNode {
  int id, a, j, i;   // id < 0: void
};
// slot idx of the candidate list: of level L (cand == nullptr) the idx-th of all (a, j, i) with j, i multiples of 2^L
__device__ inline BbsNode bbs_node(const int *__restrict__ cand, int idx, const BbsGrid &b) {
  BbsNode nd;
  if (cand) {
    nd.id = cand[idx];
    if (nd.id < 0) return nd.a = nd.j = nd.i = -1, nd;
    nd.i = nd.id % b.W;
    const int aj = nd.id / b.W;
    nd.j = aj % b.H, nd.a = aj / b.H;
    return nd;
  }
  const int ni = (b.W + (1 << b.L) - 1) >> b.L, nj = (b.H + (1 << b.L) - 1) >> b.L;
  nd.i = (idx % ni) << b.L;
  const int aj = idx / ni;
  nd.j = (aj % nj) << b.L, nd.a = aj / nj;
  nd.id = (nd.a * b.H + nd.j) * b.W + nd.i;
  return nd;
}
__device__ inline int bbs_slots(const int *__restrict__ cand, int n_root, const int *__restrict__ slots_dev) {
  return cand ? *slots_dev : n_root;
}

// The hot path.  grid = slot capacity / BBS_NODES, sized by capacity: a workgroup past the list returns.  Lane k of every
// wave holds node k of the workgroup; the candidates are sorted by yaw, so the workgroup walks the yaws a_lo .. a_hi of its
// nodes (one, where the list is long), stages that yaw's offsets in LDS chunk by chunk and every wave takes a quarter of
// the chunk: all lanes read the same LDS word (a broadcast) and gather one byte of the level's grid each, neighbouring
// nodes from neighbouring bytes.  The four partial sums of a node are added by wave 0.
__global__ __launch_bounds__(256) void k_bbs_score(const int *__restrict__ cand, int n_root, const int *__restrict__ slots_dev,
                                                    BbsGrid b, int l, const int *__restrict__ offs,
                                                    const int *__restrict__ n_dev, int cap, int *__restrict__ score,
                                                    int *__restrict__ hist) {
  __shared__ int4 chunk[BBS_CHUNK / 4];
  __shared__ int part[4][BBS_NODES];
  const int slots = bbs_slots(cand, n_root, slots_dev);
  const int first = blockIdx.x * BBS_NODES;
  if (first >= slots) return;
  const int n = min(cap, max(*n_dev, 0));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int idx = first + lane;
  BbsNode nd;
  nd.id = nd.a = nd.j = nd.i = -1;
  if (idx < slots) nd = bbs_node(cand, idx, b);
  int a_lo = nd.id >= 0 ? nd.a : 0x7FFFFFFF, a_hi = nd.a;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a_lo = min(a_lo, __shfl_xor(a_lo, o, 64));
    a_hi = max(a_hi, __shfl_xor(a_hi, o, 64));
  }
  const unsigned char *__restrict__ g = b.g + (size_t)l * b.Ws * b.Hs;
  const int x0 = nd.i + b.pad, y0 = nd.j + b.pad;
  int acc = 0;
  for (int a = a_lo; a <= a_hi; ++a) {                       // empty where every slot is void (a_hi = -1)
    const bool mine = nd.a == a;
    const int *__restrict__ row = offs + (size_t)a * cap;
    for (int c0 = 0; c0 < n; c0 += BBS_CHUNK) {
      __syncthreads();                                       // the chunk before has been read
      int4 w;
      const int p = c0 + 4 * threadIdx.x;
      w.x = p < n ? row[p] : BBS_VOID;
      w.y = p + 1 < n ? row[p + 1] : BBS_VOID;
      w.z = p + 2 < n ? row[p + 2] : BBS_VOID;
      w.w = p + 3 < n ? row[p + 3] : BBS_VOID;
      chunk[threadIdx.x] = w;
      __syncthreads();
      if (!mine) continue;
      const int q1 = min(BBS_CHUNK / 4, (n - c0 + 3) / 4);   // int4 entries that hold points
      for (int q = wave; q < q1; q += 4) {
        const int4 v = chunk[q];
        const int e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (e[k] == BBS_VOID) continue;                    // the same for every lane
          const int x = x0 + (int)(short)(e[k] & 0xFFFF), y = y0 + (e[k] >> 16);
          if ((unsigned)x < (unsigned)b.Ws && (unsigned)y < (unsigned)b.Hs) acc += g[(size_t)y * b.Ws + x];
        }
      }
    }
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && idx < slots) {
    const int s = nd.id >= 0 ? ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane] : -1;
    score[idx] = s;
    if (s >= 0) atomicAdd(&hist[s], 1);
  }
}

constexpr int BBS_THR_THREADS = 1024;
// the inclusive suffix sum of v over the workgroup's threads (thread t: the sum of threads t .. 1023) and the total
__device__ inline int bbs_suffix_sum(int v, int *wsum, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_down(v, o, 64);
    if (lane + o < 64) v += u;
  }
  if (lane == 0) wsum[wave] = v;
  __syncthreads();
  int add = 0;
  total = 0;
  for (int w = 0; w < BBS_THR_THREADS / 64; ++w) {
    if (w > wave) add += wsum[w];
    total += wsum[w];
  }
  __syncthreads();
  return v + add;
}
__device__ inline int bbs_block_max(int v, int *wsum) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  int m = wsum[0];
  for (int w = 1; w < BBS_THR_THREADS / 64; ++w) m = max(m, wsum[w]);
  __syncthreads();
  return m;
}

// One workgroup.  Thread t owns the scores [t * seg, (t + 1) * seg) of the histogram (the scores 0 .. cap).  With N the
// candidates and S those with score >= min_score: S <= F keeps them all; otherwise the cut score is the largest t with
// at least F candidates of score >= t, those above it are kept and of those at it the first `quota` in candidate order.
// The highest score dropped goes into the bound, the number dropped into the count, and the histogram is left all zero.
__global__ __launch_bounds__(BBS_THR_THREADS) void k_bbs_threshold(int *__restrict__ hist, int cap, int frontier, int min_score,
                                                                    int l, int *__restrict__ ctl, int *__restrict__ info) {
  __shared__ int wsum[BBS_THR_THREADS / 64];
  __shared__ int cut[3];                                     // the cut score, its quota, 1 where ties at the cut are dropped
  const int seg = (cap + BBS_THR_THREADS) / BBS_THR_THREADS;     // ceil((cap + 1) / threads)
  const int s0 = threadIdx.x * seg, s1 = min(cap + 1, s0 + seg);
  int all = 0, ok = 0;
  for (int s = s0; s < s1; ++s) {
    const int h = hist[s];
    all += h;
    if (s >= min_score) ok += h;
  }
  int N, S;
  (void)bbs_suffix_sum(all, wsum, N);
  const int incl = bbs_suffix_sum(ok, wsum, S);
  if (threadIdx.x == 0) cut[0] = min_score, cut[1] = 0, cut[2] = 0;
  __syncthreads();
  const bool cutting = S > frontier;
  if (cutting && incl >= frontier && incl - ok < frontier) {  // exactly one thread: the cut score lies in its segment
    int run = incl - ok;
    for (int s = s1 - 1; s >= s0; --s) {
      const int h = s >= min_score ? hist[s] : 0;
      if (run + h >= frontier) {
        cut[0] = s, cut[1] = frontier - run, cut[2] = frontier - run < h;
        break;
      }
      run += h;
    }
  }
  __syncthreads();
  const int t = cut[0], quota = cut[1], ties_dropped = cut[2];
  int hi = -1;                                               // the highest score below the cut that some candidate has
  for (int s = s0; s < s1; ++s) {
    if (s < t && hist[s] > 0) hi = s;
    hist[s] = 0;
  }
  hi = bbs_block_max(hi, wsum);
  if (threadIdx.x == 0) {
    const int kept = cutting ? frontier : S;
    ctl[BBS_C_GT] = cutting ? t : t - 1;
    ctl[BBS_C_TIE] = cutting ? t : -2;
    ctl[BBS_C_QUOTA] = quota;
    ctl[BBS_C_BOUND] = max(ctl[BBS_C_BOUND], ties_dropped ? t : hi);
    ctl[BBS_C_DROPPED] += N - kept;
    info[4 + 2 * l] = N, info[5 + 2 * l] = kept;
  }
}

// the two flags of slot idx under the level's cut: above it, at it
__device__ inline void bbs_flags(const int *__restrict__ score, const int *__restrict__ ctl, int idx, int slots, int &above,
                                 int &tie) {
  const int s = idx < slots ? score[idx] : -1;
  above = s > ctl[BBS_C_GT], tie = s == ctl[BBS_C_TIE];
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_bbs_count(const int *__restrict__ cand, int n_root, const int *__restrict__ slots_dev,
                                                           const int *__restrict__ ctl, const int *__restrict__ score, int *__restrict__ sums_above,
                                                           int *__restrict__ sums_tie) {
  __shared__ int lds_a[SCAN_BLOCK / 64], lds_t[SCAN_BLOCK / 64];
  const int slots = bbs_slots(cand, n_root, slots_dev);
  if ((int)blockIdx.x * SCAN_BLOCK >= slots) return;
  int above, tie;
  bbs_flags(score, ctl, blockIdx.x * SCAN_BLOCK + threadIdx.x, slots, above, tie);
  compact_count(above, lds_a, sums_above);
  compact_count(tie, lds_t, sums_tie);
}

// A node is kept where it is above the cut, or at it with fewer than `quota` such nodes before it; its place among the
// kept is (nodes above the cut before it) + min(nodes at the cut before it, quota).  Level l > 0: the kept node at place k
// writes its four children into slots 4k .. 4k + 3 of `next` ((dj, di) = (0,0), (0,1), (1,0), (1,1); outside the grid: -1).
// Level 0: next[k] is the leaf's id and next[frontier + k] its score.  The last workgroup of the list publishes the slots
// of the next list; an empty list is published by workgroup 0.
__global__ __launch_bounds__(SCAN_BLOCK) void k_bbs_write(const int *__restrict__ cand, int n_root, const int *__restrict__ slots_dev,
                                                           const int *__restrict__ ctl, int *__restrict__ slots_out, BbsGrid b, int l, const int *__restrict__ score,
                                                           const int *__restrict__ sums_above, const int *__restrict__ sums_tie,
                                                           int frontier, int *__restrict__ next, int *__restrict__ trace) {
  __shared__ int lds_a[SCAN_BLOCK / 64], lds_t[SCAN_BLOCK / 64], wo_a[SCAN_BLOCK / 64], wo_t[SCAN_BLOCK / 64];
  const int slots = bbs_slots(cand, n_root, slots_dev);
  if (slots <= 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *slots_out = 0;
    return;
  }
  if ((int)blockIdx.x * SCAN_BLOCK >= slots) return;
  const int base_a = compact_base(sums_above, lds_a), base_t = compact_base(sums_tie, lds_t);
  const int idx = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  const int quota = ctl[BBS_C_QUOTA];
  int above, tie, upto_a, upto_t;
  bbs_flags(score, ctl, idx, slots, above, tie);
  const int ra = compact_rank(base_a, above, wo_a, upto_a);
  const int rt = compact_rank(base_t, tie, wo_t, upto_t);
  const int k = ra + min(rt, quota);
  const BbsNode nd = idx < slots ? bbs_node(cand, idx, b) : BbsNode{-1, -1, -1, -1};
  int *tr = trace ? trace + (size_t)l * 5 * frontier : nullptr;     // the level's candidate slots [4F], then its kept nodes [F]
  if (tr && idx < slots) tr[idx] = nd.id;
  if ((above || (tie && rt < quota)) && k < frontier) {
    if (tr) tr[4 * frontier + k] = nd.id;
    if (l > 0) {
      const int h = 1 << (l - 1);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = nd.i + (c & 1) * h, j = nd.j + (c >> 1) * h;
        next[4 * k + c] = (i < b.W && j < b.H) ? (nd.a * b.H + j) * b.W + i : -1;
      }
    } else {
      next[k] = nd.id, next[frontier + k] = score[idx];
    }
  }
  if ((int)blockIdx.x == (slots - 1) / SCAN_BLOCK && threadIdx.x == 0) {
    const int kept = min(upto_a + min(upto_t, quota), frontier);
    *slots_out = l > 0 ? 4 * kept : kept;
  }
}

// ---- the result ----------------------------------------------------------------------------------------------------------
// true where leaf (s, i) comes before leaf (bs, bi) in the order (score descending, id ascending); bi < 0: no leaf yet
__device__ inline bool bbs_top_before(int s, int i, int bs, int bi) { return bi < 0 || s > bs || (s == bs && i < bi); }

// pose of leaf (a, j, i): Trans(r (i0 + i), r (j0 + j), 0) Rz(yaw a) T_up.  Rows 0 and 1 are c U0 - s U1 and s U0 + c U1
// per entry, the translation is added to entries 3 and 7, rows 2 and 3 are T_up's
__device__ inline double bbs_pose_entry(const LocPose &U, double c, double s, double tx, double ty, int e) {
  const int col = e & 3;
  if (e < 4) {
    const double v = loc_add(loc_mul(c, U.m[col]), -loc_mul(s, U.m[4 + col]));
    return col == 3 ? loc_add(v, tx) : v;
  }
  if (e < 8) {
    const double v = loc_add(loc_mul(s, U.m[col]), loc_mul(c, U.m[4 + col]));
    return col == 3 ? loc_add(v, ty) : v;
  }
  return U.m[e];
}

// One workgroup, as k_ndt_top: round r takes the first leaf, in the order (score descending, id ascending), that comes
// after the leaf of round r - 1.  Slots past the last leaf get index -1, score 0 and the pose of slot 0 (T_up where there
// is no leaf).  certified = the leading results with score > the bound; the info words are completed here.
__global__ __launch_bounds__(NDT_TOP_THREADS) void k_bbs_top(const int *__restrict__ leaves, int frontier, const int *__restrict__ n_leaf_dev,
                                                              const int *__restrict__ ctl,
                                                              BbsGrid b, LocPose T_up, double r, int i0, int j0,
                                                              const double *__restrict__ yaw_cs, int k,
                                                              int *__restrict__ top_index, int *__restrict__ top_score,
                                                              double *__restrict__ T_top, int *__restrict__ n_top,
                                                              int *__restrict__ info) {
  __shared__ int ws[NDT_TOP_THREADS / 64], wi[NDT_TOP_THREADS / 64];
  __shared__ int pick_s, pick_i;
  __shared__ double first_pose[16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n_leaf = min(*n_leaf_dev, frontier), bound = ctl[BBS_C_BOUND];
  k = min(k, SPS_NDT_MAX_HYP);
  int ps = 0x7FFFFFFF, pi = -1, filled = 0, certified = 0;   // the previous pick; (max, -1) comes before every leaf
  if (t < 16) first_pose[t] = T_up.m[t];
  for (int rr = 0; rr < k; ++rr) {
    int bs = 0, bi = -1;
    for (int p = t; p < n_leaf; p += NDT_TOP_THREADS) {
      const int id = leaves[p], s = leaves[frontier + p];
      if (!(s < ps || (s == ps && id > pi))) continue;       // taken in an earlier round
      if (bbs_top_before(s, id, bs, bi)) bs = s, bi = id;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int os = __shfl_xor(bs, o, 64), oi = __shfl_xor(bi, o, 64);
      if (oi >= 0 && bbs_top_before(os, oi, bs, bi)) bs = os, bi = oi;
    }
    if (lane == 0) ws[wave] = bs, wi[wave] = bi;
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < NDT_TOP_THREADS / 64; ++w)
        if (wi[w] >= 0 && bbs_top_before(ws[w], wi[w], bs, bi)) bs = ws[w], bi = wi[w];
      pick_s = bs, pick_i = bi;
    }
    __syncthreads();
    ps = pick_s, pi = pick_i;
    __syncthreads();                                         // the next round writes ws, wi and the pick again
    if (pi < 0) break;                                       // the same for every thread
    if (ps > bound && certified == rr) certified = rr + 1;
    if (t == 0) top_index[rr] = pi, top_score[rr] = ps;
    if (t < 16) {
      const int i = pi % b.W, aj = pi / b.W;
      const int j = aj % b.H, a = aj / b.H;
      const double e = bbs_pose_entry(T_up, yaw_cs[2 * a], yaw_cs[2 * a + 1], loc_mul(r, (double)(i0 + i)),
                                      loc_mul(r, (double)(j0 + j)), t);
      T_top[(size_t)rr * 16 + t] = e;
      if (rr == 0) first_pose[t] = e;
    }
    filled = rr + 1;
  }
  __syncthreads();
  for (int rr = filled; rr < k; ++rr) {
    if (t == 0) top_index[rr] = -1, top_score[rr] = 0;
    if (t < 16) T_top[(size_t)rr * 16 + t] = first_pose[t];
  }
  if (t == 0) {
    *n_top = filled;
    info[0] = certified, info[1] = bound, info[2] = ctl[BBS_C_DROPPED];
  }
}

#pragma clang fp contract(fast)
