// lts_kernels.inc.h -- the LTS baseline (SPCTReg offset-attention regressor + its range-image loader) on gfx950.
// Section of sps_hip.hip (inside its anonymous namespace).  Replaces, in the reference tree,
//   c_ws/src/inference_model/lts_filter/scripts/loader.py:36-59        range-image projection  (k_lts_proj_*)
//   c_ws/src/inference_model/lts_filter/scripts/transformer.py         SPCTReg forward          (k_lts_gemm, k_lts_attn_*)
// Layout: activations are point-major f32 rows [B*N, C] (row b*N + n = point n of window b); the four OA outputs are
// column blocks of one [B*N, 512] buffer, so torch.cat([x1..x4]) costs nothing.  Every reduction runs in a fixed
// order and no kernel here uses a float atomic: a forward is bit-reproducible.  The N x N attention matrix is never
// stored: pass A keeps per-query (max, 1/sum) of the row softmax, pass B recomputes the energies per key block.

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int LTS_SLICES = 1024;
constexpr int LTS_QV = 160;   // row of the qv buffer: q (32) | v (128)
constexpr int LTS_PL = 129;   // row of the pass-B partials: sum_i v[i][c] P[i][j] (128) | sum_i P[i][j]

// ---- projection ---------------------------------------------------------------------------------------------------
struct LtsLidar {
  int beams, window;
  float fov_down, theta_res;  // f32 as numpy sees them (weak Python scalars): fov_down, f32((up - down) / (beams - 1))
};

// order-preserving 32-bit image of a float (-0.0 folded onto +0.0, as np.unique compares)
__device__ inline uint32_t lts_ord(float f) {
  if (f == 0.f) f = 0.f;
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// cell (beam * 1024 + slice) of a row, -1 = dropped (s == -1), -2 = error (status bit 1: theta index out of the
// image, bit 2: NaN coordinate).  loader.py:45-53 in float32 and numpy's operation order, no contraction.
__device__ inline int lts_cell(const float *p, const LtsLidar L, int *status) {
#pragma clang fp contract(off)
  const float x = p[0], y = p[1], z = p[2], s = p[3];
  if (s == -1.f) return -1;
  if (isnan(x) || isnan(y) || isnan(z)) {
    if (status) atomicOr(status, 2);
    return -2;
  }
  const float pi = 3.14159265358979323846f;
  const float theta = atan2f(z, sqrtf(x * x + y * y)) * 180.f / pi;
  const float phi = atan2f(y, x) * 180.f / pi;
  int ti = (int)floorf((theta - L.fov_down) / L.theta_res);
  int pj = (int)floorf(phi / (360.f / LTS_SLICES));
  if (ti < -L.beams || ti >= L.beams || pj < -LTS_SLICES || pj >= LTS_SLICES) {  // IndexError in the reference
    if (status) atomicOr(status, 1);
    return -2;
  }
  if (ti < 0) ti += L.beams;  // Python negative index
  if (pj < 0) pj += LTS_SLICES;
  return ti * LTS_SLICES + pj;
}

__device__ inline unsigned long long lts_key(float a, float b) {
  return ((unsigned long long)lts_ord(a) << 32) | lts_ord(b);
}

// The reference keeps, per cell, the last of np.unique's lexicographically sorted rows: the largest (x, y, z, s).
// Selected with integer atomics in two rounds: max (x, y) per cell, then max (z, s) among the rows that won round 1.
__global__ void k_lts_proj_xy(const float *pts, int64_t ld, int n, LtsLidar L, unsigned long long *kxy, int *status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *p = pts + (int64_t)i * ld;
  const int cell = lts_cell(p, L, status);
  if (cell >= 0) atomicMax(&kxy[cell], lts_key(p[0], p[1]));
}

__global__ void k_lts_proj_zs(const float *pts, int64_t ld, int n, LtsLidar L, const unsigned long long *kxy,
                              unsigned long long *kzs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *p = pts + (int64_t)i * ld;
  const int cell = lts_cell(p, L, nullptr);
  if (cell >= 0 && kxy[cell] == lts_key(p[0], p[1])) atomicMax(&kzs[cell], lts_key(p[2], p[3]));
}

// every winning row writes the same values (rows equal up to the sign of a zero)
__global__ void k_lts_proj_write(const float *pts, int64_t ld, int n, LtsLidar L, const unsigned long long *kxy,
                                 const unsigned long long *kzs, float *frame) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *p = pts + (int64_t)i * ld;
  const int cell = lts_cell(p, L, nullptr);
  if (cell >= 0 && kxy[cell] == lts_key(p[0], p[1]) && kzs[cell] == lts_key(p[2], p[3])) {
    float *f = frame + (int64_t)cell * 4;
    f[0] = p[0];
    f[1] = p[1];
    f[2] = p[2];
    f[3] = p[3];
  }
}

// frame [beams][1024][4] -> network input x [windows][3][N] and metric rows [windows * N][6] = (0, x, y, z, 1, s);
// window w is frame[:, wW:(w+1)W].reshape(-1, 4) (loader.py:64-68): point n = beam * W + column in the window
__global__ void k_lts_proj_unpack(const float *frame, LtsLidar L, float *x, float *rows) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= L.beams * LTS_SLICES) return;
  const int beam = cell / LTS_SLICES, col = cell % LTS_SLICES;
  const int w = col / L.window, N = L.beams * L.window;
  const int nn = beam * L.window + col % L.window;
  const float *f = frame + (int64_t)cell * 4;
  if (x) {
    float *xw = x + (int64_t)w * 3 * N + nn;
    xw[0] = f[0];
    xw[N] = f[1];
    xw[2 * N] = f[2];
  }
  if (rows) {
    float *r = rows + ((int64_t)w * N + nn) * 6;
    r[0] = 0.f;
    r[1] = f[0];
    r[2] = f[1];
    r[3] = f[2];
    r[4] = 1.f;
    r[5] = f[3];
  }
}

// ---- pointwise convolutions --------------------------------------------------------------------------------------
// embedding.conv1 (3 -> 128, BN folded) + ReLU, reading the caller's [B, 3, N] input
__global__ void k_lts_embed1(const float *x, int B, int N, const float *W, const float *bias, float *out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * N * 128) return;
  const int o = (int)(t & 127);
  const int64_t r = t >> 7;
  const int64_t b = r / N, nn = r % N;
  const float *xp = x + b * 3 * N + nn;
  float v = bias[o];
  v = fmaf(W[o * 3 + 0], xp[0], v);
  v = fmaf(W[o * 3 + 1], xp[N], v);
  v = fmaf(W[o * 3 + 2], xp[2 * N], v);
  out[t] = fmaxf(v, 0.f);
}

enum LtsEpi { LE_BIAS = 0, LE_RELU, LE_RES_RELU, LE_LRELU_POOL, LE_SILU, LE_SILU_WBIAS };

struct LtsGemm {
  const float *A;  // [B*M, K] rows with stride lda (window b starts at row b*M)
  int64_t lda;
  const float *W;  // [Nout, K] row-major (BN folded)
  const float *bias;
  float *C;
  int64_t ldc;
  const float *R;  // residual rows (LE_RES_RELU), stride ldr
  int64_t ldr;
  const float *wbias;  // [B, Nout] per-window bias (LE_SILU_WBIAS)
  float *pmax, *psum;  // [B, mtiles, Nout] column partials of the tile (LE_LRELU_POOL)
  int M, Nout, K, mtiles;
};

constexpr int LG_T = 128, LG_K = 16, LG_PAD = 4;

__device__ inline int lts_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }  // 32x32 C/D row map

// C[b*M + m, o] = epi(sum_k A[b*M + m, k] W[o, k]): 128 x 128 tile per workgroup, 4 waves of 64 x 64 (2 x 2 tiles
// of v_mfma_f32_32x32x2_f32, exact f32 products), K staged through LDS 16 at a time, next slice prefetched to
// registers.  K % 16 == 0, lda % 4 == 0 (host checks).
template <int EPI>
__global__ __launch_bounds__(256) void k_lts_gemm(LtsGemm g) {
  __shared__ float As[LG_K][LG_T + LG_PAD], Ws[LG_K][LG_T + LG_PAD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  const int b = blockIdx.z, m0 = blockIdx.y * LG_T, n0 = blockIdx.x * LG_T;
  const int lr = tid >> 1, lk = (tid & 1) * 8;
  const bool arow = m0 + lr < g.M, wrow = n0 + lr < g.Nout;
  const float *ap = g.A + ((int64_t)b * g.M + (arow ? m0 + lr : 0)) * g.lda + lk;
  const float *wp = g.W + (int64_t)(wrow ? n0 + lr : 0) * g.K + lk;
  const floatx4 z4 = {0.f, 0.f, 0.f, 0.f};
  floatx4 ra0 = z4, ra1 = z4, rw0 = z4, rw1 = z4;
  auto fetch = [&](int k0) {
    if (arow) {
      ra0 = *(const floatx4 *)(ap + k0);
      ra1 = *(const floatx4 *)(ap + k0 + 4);
    }
    if (wrow) {
      rw0 = *(const floatx4 *)(wp + k0);
      rw1 = *(const floatx4 *)(wp + k0 + 4);
    }
  };
  floatx16 acc[2][2];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  fetch(0);
  for (int k0 = 0; k0 < g.K; k0 += LG_K) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      As[lk + q][lr] = ra0[q];
      As[lk + 4 + q][lr] = ra1[q];
      Ws[lk + q][lr] = rw0[q];
      Ws[lk + 4 + q][lr] = rw1[q];
    }
    __syncthreads();
    if (k0 + LG_K < g.K) fetch(k0 + LG_K);
#pragma unroll
    for (int s = 0; s < LG_K / 2; ++s) {
      const float a0 = As[2 * s + h][wm * 64 + c], a1 = As[2 * s + h][wm * 64 + 32 + c];
      const float b0 = Ws[2 * s + h][wn * 64 + c], b1 = Ws[2 * s + h][wn * 64 + 32 + c];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }

  float pm[2] = {-INFINITY, -INFINITY}, ps[2] = {0.f, 0.f};
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    const int col = n0 + wn * 64 + tj * 32 + c;
    const bool cok = col < g.Nout;
    float bias = 0.f;
    if (cok) {
      if (EPI == LE_SILU_WBIAS) bias = g.wbias[(int64_t)b * g.Nout + col];
      else if (g.bias) bias = g.bias[col];
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 + ti * 32 + lts_row(r, h);
        if (!cok || m >= g.M) continue;
        const int64_t row = (int64_t)b * g.M + m;
        float v = acc[ti][tj][r] + bias;
        if (EPI == LE_RELU) v = fmaxf(v, 0.f);
        if (EPI == LE_RES_RELU) v = g.R[row * g.ldr + col] + fmaxf(v, 0.f);
        if (EPI == LE_LRELU_POOL) {
          v = v > 0.f ? v : 0.2f * v;
          pm[tj] = fmaxf(pm[tj], v);
          ps[tj] += v;
        }
        if (EPI == LE_SILU || EPI == LE_SILU_WBIAS) v = v / (1.f + expf(-v));
        g.C[row * g.ldc + col] = v;
      }
    }
  }
  if constexpr (EPI == LE_LRELU_POOL) {
    __shared__ float rmax[2][LG_T], rsum[2][LG_T];
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const float om = __shfl_xor(pm[tj], 32), os = __shfl_xor(ps[tj], 32);
      if (h == 0) {
        rmax[wm][wn * 64 + tj * 32 + c] = fmaxf(pm[tj], om);
        rsum[wm][wn * 64 + tj * 32 + c] = ps[tj] + os;
      }
    }
    __syncthreads();
    if (tid < LG_T && n0 + tid < g.Nout) {
      const int64_t o = ((int64_t)b * g.mtiles + blockIdx.y) * g.Nout + n0 + tid;
      g.pmax[o] = fmaxf(rmax[0][tid], rmax[1][tid]);
      g.psum[o] = rsum[0][tid] + rsum[1][tid];
    }
  }
}

// linear1's global max and mean over the N points of a window, from the tile partials in tile order
__global__ void k_lts_pool(const float *pmax, const float *psum, int mtiles, int Nout, int M, float *gmax, float *gmean) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (o >= Nout) return;
  float m = -INFINITY;
  double s = 0.0;
  for (int t = 0; t < mtiles; ++t) {
    const int64_t i = ((int64_t)b * mtiles + t) * Nout + o;
    m = fmaxf(m, pmax[i]);
    s += (double)psum[i];
  }
  gmax[(int64_t)b * Nout + o] = m;
  gmean[(int64_t)b * Nout + o] = (float)(s / M);
}

// linear2's per-window bias: the max / mean thirds of the 6144 -> 512 conv act on features constant over the window,
// wb[b, o] = bias[o] + W[o, 2048:4096] . max[b] + W[o, 4096:6144] . mean[b]   (one wave per (b, o), fixed lane order)
__global__ __launch_bounds__(256) void k_lts_wbias(const float *Wp, const float *bias, const float *gmax, const float *gmean,
                                                   int B, float *wb) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= B * 512) return;
  const int b = t / 512, o = t % 512;
  const float *w = Wp + (int64_t)o * 4096;
  const float *mx = gmax + (int64_t)b * 2048, *mn = gmean + (int64_t)b * 2048;
  float s = 0.f;
  for (int k = lane; k < 2048; k += 64) s = fmaf(w[k], mx[k], fmaf(w[2048 + k], mn[k], s));
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if (lane == 0) wb[t] = bias[o] + s;
}

// convs (256 -> 1) + sigmoid
__global__ void k_lts_head(const float *h3, int64_t rows, const float *w, float b0, float *scores) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const floatx4 *p = (const floatx4 *)(h3 + r * 256);
  const floatx4 *q = (const floatx4 *)w;
  float s = b0;
  for (int k = 0; k < 64; ++k) {
    const floatx4 a = p[k], c = q[k];
    s = fmaf(a[0], c[0], s);
    s = fmaf(a[1], c[1], s);
    s = fmaf(a[2], c[2], s);
    s = fmaf(a[3], c[3], s);
  }
  scores[r] = 1.f / (1.f + expf(-s));
}

// ---- offset attention ----------------------------------------------------------------------------------------------
// energy E = Q Q^T (q_conv and k_conv share one weight, transformer.py:40-42).  A 32 x 32 energy tile is one chain of
// sixteen v_mfma_f32_32x32x2_f32 over the 32 q channels; in step s lane half h supplies channel 16h + s, so a lane
// loads 16 contiguous floats of its row.  Both passes build their tiles with this function: the energies of pass B
// are bit-identical to the ones pass A took the row maxima of.
__device__ inline void lts_load_q(const float *Q, int row, bool ok, int h, float (&q)[16]) {
  if (ok) {
    const floatx4 *p = (const floatx4 *)(Q + (int64_t)row * LTS_QV + 16 * h);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const floatx4 v = p[t];
      q[4 * t] = v[0];
      q[4 * t + 1] = v[1];
      q[4 * t + 2] = v[2];
      q[4 * t + 3] = v[3];
    }
  } else {
#pragma unroll
    for (int s = 0; s < 16; ++s) q[s] = 0.f;
  }
}

__device__ inline floatx16 lts_energy(const float (&a)[16], const float (&b)[16]) {
  floatx16 e;
  for (int r = 0; r < 16; ++r) e[r] = 0.f;
#pragma unroll
  for (int s = 0; s < 16; ++s) e = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], e, 0, 0, 0);
  return e;
}

// pass A: per query i, m_i = max_j E_ij and 1 / l_i, l_i = sum_j exp(E_ij - m_i) (softmax(dim=-1)), online over key
// tiles.  One wave per 32 queries; the tile is E^T (keys on the rows), so a lane's 16 registers are 16 keys of its query.
__global__ __launch_bounds__(64) void k_lts_attn_stats(const float *qv, int N, float *mrow, float *rlrow) {
  const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
  const int b = blockIdx.y, i = blockIdx.x * 32 + c;
  const float *Q = qv + (int64_t)b * N * LTS_QV;
  float qb[16];
  lts_load_q(Q, i, i < N, h, qb);
  float m = -INFINITY, l = 0.f;
  for (int j0 = 0; j0 < N; j0 += 32) {
    float ka[16];
    lts_load_q(Q, j0 + c, j0 + c < N, h, ka);
    const floatx16 e = lts_energy(ka, qb);  // e[r] = E[j0 + row(r, h)][i]
    float tm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (j0 + lts_row(r, h) < N) tm = fmaxf(tm, e[r]);
    const float mn = fmaxf(m, tm);
    if (mn != -INFINITY) {
      l *= __expf(m - mn);
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (j0 + lts_row(r, h) < N) l += __expf(e[r] - mn);
      m = mn;
    }
  }
  const float mo = __shfl_xor(m, 32), lo = __shfl_xor(l, 32);
  const float M = fmaxf(m, mo);
  const float L = (m == -INFINITY ? 0.f : l * __expf(m - M)) + (mo == -INFINITY ? 0.f : lo * __expf(mo - M));
  if (h == 0 && i < N) {
    mrow[(int64_t)b * N + i] = M;
    rlrow[(int64_t)b * N + i] = 1.f / L;
  }
}

// pass B: per key j, over the queries i of this split: P_ij = exp(E_ij - m_i) / l_i, column sum sum_i P_ij and
// sum_i v_i P_ij (x_r before the column normalisation, transformer.py:60-63).  One wave per 32 keys and all 128 value
// channels: the energy tile (queries on the rows) is, register for register, the A operand of the P^T V product.
__global__ __launch_bounds__(64) void k_lts_attn_out(const float *qv, int N, const float *mrow, const float *rlrow,
                                                     int rows_per_split, float *part, int64_t split_stride) {
  const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
  const int b = blockIdx.y, j0 = blockIdx.x * 32, split = blockIdx.z;
  const float *Q = qv + (int64_t)b * N * LTS_QV;
  const float *mb = mrow + (int64_t)b * N, *lb = rlrow + (int64_t)b * N;
  float kq[16];
  lts_load_q(Q, j0 + c, j0 + c < N, h, kq);
  floatx16 o[4];
  for (int t = 0; t < 4; ++t)
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float cs = 0.f;
  const int i_begin = split * rows_per_split, i_end = min(N, i_begin + rows_per_split);
  for (int i0 = i_begin; i0 < i_end; i0 += 32) {
    float qa[16];
    lts_load_q(Q, i0 + c, i0 + c < i_end, h, qa);
    const floatx16 e = lts_energy(qa, kq);  // e[r] = E[i0 + row(r, h)][j0 + c]
    float p[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + lts_row(r, h);
      p[r] = i < i_end ? __expf(e[r] - mb[i]) * lb[i] : 0.f;
      cs += p[r];
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int i = i0 + lts_row(s, h);
      const float *vr = Q + (int64_t)(i < i_end ? i : 0) * LTS_QV + 32 + c;
      const bool ok = i < i_end;
#pragma unroll
      for (int t = 0; t < 4; ++t) o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[s], ok ? vr[32 * t] : 0.f, o[t], 0, 0, 0);
    }
  }
  const float cst = cs + __shfl_xor(cs, 32);
  float *pp = part + (int64_t)split * split_stride + (int64_t)b * N * LTS_PL;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + lts_row(r, h);  // o[t][r] = sum_i P[i][j] v[i][32t + c]
      if (j < N) pp[(int64_t)j * LTS_PL + 32 * t + c] = o[t][r];
    }
  if (h == 0 && j0 + c < N) pp[(int64_t)(j0 + c) * LTS_PL + 128] = cst;
}

// splits in order; x_r = (sum_i v_i P_ij) / (1e-9 + sum_i P_ij); d = x - x_r (the input of trans_conv)
__global__ void k_lts_attn_combine(const float *part, int splits, int64_t split_stride, int64_t rows, const float *x,
                                   int64_t ldx, float *d) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * 128) return;
  const int64_t r = t >> 7;
  const int ch = (int)(t & 127);
  float o = 0.f, s = 0.f;
  for (int k = 0; k < splits; ++k) {
    const float *p = part + k * split_stride + r * LTS_PL;
    o += p[ch];
    s += p[128];
  }
  d[t] = x[r * ldx + ch] - o / (1e-9f + s);
}
