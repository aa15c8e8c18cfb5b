// lts_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block): the LTS baseline's handle, weight
// folding and launch sequence (kernels: lts_kernels.inc.h; ABI: the "LTS baseline" section of include/sps_hip.h).
//
// Launch list of one forward of B windows x N points (28 launches, none of them synchronising):
//   k_lts_embed1, k_lts_gemm<RELU>                                   embedding (conv1 / conv2, BN folded)
//   4 x [ k_lts_gemm<BIAS> (q | v), k_lts_attn_stats, k_lts_attn_out, k_lts_attn_combine, k_lts_gemm<RES_RELU> ]
//   k_lts_gemm<LRELU_POOL>, k_lts_pool, k_lts_wbias                  linear1 + global max / mean, linear2's max/mean third
//   k_lts_gemm<SILU_WBIAS>, k_lts_gemm<SILU>, k_lts_head             linear2, linear3, convs + sigmoid

extern "C++" {
namespace {

struct LtsTensor {
  std::string name;
  int ndim;
  int64_t shape[3];
  int64_t offset, numel;
};

// the reference's state_dict, in its order (transformer.py:5-140; num_batches_tracked travels as one float)
const std::vector<LtsTensor> &lts_spec() {
  static const std::vector<LtsTensor> spec = [] {
    std::vector<LtsTensor> v;
    int64_t off = 0;
    auto add = [&](const std::string &n, std::initializer_list<int64_t> sh) {
      LtsTensor t{n, (int)sh.size(), {1, 1, 1}, off, 1};
      int d = 0;
      for (int64_t s : sh) {
        t.shape[d++] = s;
        t.numel *= s;
      }
      off += t.numel;
      v.push_back(t);
    };
    auto bn = [&](const std::string &p, int64_t c) {
      add(p + ".weight", {c});
      add(p + ".bias", {c});
      add(p + ".running_mean", {c});
      add(p + ".running_var", {c});
      add(p + ".num_batches_tracked", {});
    };
    add("embedding.conv1.weight", {128, 3, 1});
    add("embedding.conv2.weight", {128, 128, 1});
    bn("embedding.bn1", 128);
    bn("embedding.bn2", 128);
    for (int k = 1; k <= 4; ++k) {
      const std::string p = "sa" + std::to_string(k);
      add(p + ".q_conv.weight", {32, 128, 1});
      add(p + ".k_conv.weight", {32, 128, 1});
      add(p + ".v_conv.weight", {128, 128, 1});
      add(p + ".v_conv.bias", {128});
      add(p + ".trans_conv.weight", {128, 128, 1});
      add(p + ".trans_conv.bias", {128});
      bn(p + ".after_norm", 128);
    }
    add("linear1.0.weight", {2048, 512, 1});
    bn("linear1.1", 2048);
    add("linear2.0.weight", {512, 6144, 1});
    add("linear2.0.bias", {512});
    bn("linear2.1", 512);
    add("linear3.0.weight", {256, 512, 1});
    add("linear3.0.bias", {256});
    bn("linear3.1", 256);
    add("convs.weight", {1, 256, 1});
    add("convs.bias", {1});
    return v;
  }();
  return spec;
}

int64_t lts_numel() {
  const LtsTensor &t = lts_spec().back();
  return t.offset + t.numel;
}

// device weight layout (floats), BN folded: W' = W * g / sqrt(var + 1e-5), b' = (b - mean) * g / sqrt(var + 1e-5) + beta
struct LtsW {
  int64_t e1w, e1b, e2w, e2b, qvw[4], qvb[4], tw[4], tb[4], l1w, l1b, l2w, l2p, l2b, l3w, l3b, hw, hb, total;
};

LtsW lts_wlayout() {
  LtsW L{};
  int64_t o = 0;
  auto take = [&](int64_t n) {
    const int64_t r = o;
    o += (n + 63) & ~int64_t(63);  // 256-byte aligned tensors (float4 loads)
    return r;
  };
  L.e1w = take(128 * 3);
  L.e1b = take(128);
  L.e2w = take(128 * 128);
  L.e2b = take(128);
  for (int k = 0; k < 4; ++k) {
    L.qvw[k] = take(LTS_QV * 128);
    L.qvb[k] = take(LTS_QV);
    L.tw[k] = take(128 * 128);
    L.tb[k] = take(128);
  }
  L.l1w = take(2048 * 512);
  L.l1b = take(2048);
  L.l2w = take(512 * 2048);
  L.l2p = take(512 * 4096);
  L.l2b = take(512);
  L.l3w = take(256 * 512);
  L.l3b = take(256);
  L.hw = take(256);
  L.hb = take(64);
  L.total = o;
  return L;
}

}  // namespace
}  // extern "C++"

extern "C++" {
struct sps_lts {
  int device = 0;
  float *w = nullptr;  // folded weights (LtsW layout)
  LtsW L{};
  float head_bias = 0.f;
  int *status = nullptr;  // sticky device status of sps_lts_project (bit 0 theta index out of range, bit 1 NaN)
  unsigned long long *keys = nullptr;  // projection: 2 x 32 x 1024 cell keys
  // workspace for `cap` rows (B * N)
  int64_t cap = 0, cap_b = 0;
  std::vector<void *> ws;
  float *emb = nullptr, *qv = nullptr, *d = nullptr, *cat = nullptr, *mrow = nullptr, *rl = nullptr, *part = nullptr;
  float *y1 = nullptr, *h2 = nullptr, *h3 = nullptr, *pmax = nullptr, *psum = nullptr, *gmax = nullptr, *gmean = nullptr,
        *wb = nullptr;
  int64_t last_b = 0, last_n = 0;  // the forward the taps belong to
};
}  // extern "C++"

extern "C++" {
namespace {

constexpr int LTS_MAX_SPLITS = 8;

void lts_free_ws(sps_lts *h) {
  for (void *p : h->ws) (void)hipFree(p);
  h->ws.clear();
  h->cap = h->cap_b = 0;
}

int lts_reserve(sps_lts *h, int64_t B, int64_t N) {
  const int64_t rows = B * N;
  if (rows <= h->cap && B <= h->cap_b) return SPS_OK;
  (void)hipDeviceSynchronize();  // forwards in flight may still use the old workspace
  lts_free_ws(h);
  const int64_t R = std::max(rows, h->cap), Bc = std::max(B, h->cap_b);
  const int64_t mt = (N + LG_T - 1) / LG_T;
  const int64_t mtiles_rows = std::max<int64_t>(Bc * mt, (R + LG_T - 1) / LG_T + Bc);
  auto get = [&](float **p, int64_t n) -> bool {
    void *q = nullptr;
    if (hipMalloc(&q, (size_t)std::max<int64_t>(n, 1) * sizeof(float)) != hipSuccess) return false;
    h->ws.push_back(q);
    *p = (float *)q;
    return true;
  };
  const bool ok = get(&h->emb, R * 128) && get(&h->qv, R * LTS_QV) && get(&h->d, R * 128) && get(&h->cat, R * 512) &&
                  get(&h->mrow, R) && get(&h->rl, R) && get(&h->part, (int64_t)LTS_MAX_SPLITS * R * LTS_PL) &&
                  get(&h->y1, R * 2048) && get(&h->h2, R * 512) && get(&h->h3, R * 256) &&
                  get(&h->pmax, mtiles_rows * 2048) && get(&h->psum, mtiles_rows * 2048) && get(&h->gmax, Bc * 2048) &&
                  get(&h->gmean, Bc * 2048) && get(&h->wb, Bc * 512);
  if (!ok) {
    (void)hipGetLastError();
    lts_free_ws(h);
    return fail(SPS_ERR_NOMEM, "LTS workspace for %lld rows does not fit the device", (long long)R);
  }
  h->cap = R;
  h->cap_b = Bc;
  return SPS_OK;
}

template <int EPI>
void lts_gemm(hipStream_t st, int B, const LtsGemm &g) {
  dim3 grid((unsigned)((g.Nout + LG_T - 1) / LG_T), (unsigned)((g.M + LG_T - 1) / LG_T), (unsigned)B);
  hipLaunchKernelGGL(k_lts_gemm<EPI>, grid, dim3(256), 0, st, g);
}

LtsGemm lts_g(const float *A, int64_t lda, const float *W, const float *bias, float *C, int64_t ldc, int M, int Nout, int K) {
  LtsGemm g{};
  g.A = A;
  g.lda = lda;
  g.W = W;
  g.bias = bias;
  g.C = C;
  g.ldc = ldc;
  g.M = M;
  g.Nout = Nout;
  g.K = K;
  return g;
}

bool lts_lidar(int lidar, LtsLidar *L) {
  // loader.py:13-28 (the reference's numbers as they are); theta_res formed in f64, rounded to f32 by numpy
  if (lidar == 0) {
    *L = LtsLidar{16, 128, -16.8f, (float)((16.8 - -16.8) / 15.0)};
    return true;
  }
  if (lidar == 1) {
    *L = LtsLidar{32, 64, -10.f, (float)((30.0 - -10.0) / 31.0)};
    return true;
  }
  return false;
}

}  // namespace
}  // extern "C++"

int sps_lts_num_tensors(void) { return (int)lts_spec().size(); }

int sps_lts_tensor_info(int idx, char *name, int name_cap, int64_t *offset, int64_t *numel, int64_t *shape, int *ndim) {
  const auto &s = lts_spec();
  if (idx < 0 || idx >= (int)s.size()) return fail(SPS_ERR_INVALID, "tensor index %d out of range", idx);
  const LtsTensor &t = s[idx];
  if (name && name_cap > 0) snprintf(name, (size_t)name_cap, "%s", t.name.c_str());
  if (offset) *offset = t.offset;
  if (numel) *numel = t.numel;
  if (shape)
    for (int d = 0; d < 3; ++d) shape[d] = d < t.ndim ? t.shape[d] : 0;
  if (ndim) *ndim = t.ndim;
  return SPS_OK;
}

int64_t sps_lts_numel(void) { return lts_numel(); }

int sps_lts_lidar_info(int lidar, int *beams, int *window, int *num_windows) {
  LtsLidar L;
  if (!lts_lidar(lidar, &L)) return fail(SPS_ERR_INVALID, "lidar must be 0 (vlp-16) or 1 (hdl-32)");
  if (beams) *beams = L.beams;
  if (window) *window = L.window;
  if (num_windows) *num_windows = LTS_SLICES / L.window;
  return SPS_OK;
}

int sps_lts_create(int device, const float *blob, int64_t numel, sps_lts **out) {
  if (!out) return fail(SPS_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!blob) {  // projection-only handle (Loader): no weights, sps_lts_forward fails
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<sps_lts> h(new sps_lts);
    h->device = device;
    if (hipMalloc(&h->status, sizeof(int)) != hipSuccess ||
        hipMalloc(&h->keys, sizeof(unsigned long long) * 2 * 32 * LTS_SLICES) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(h->status);
      (void)hipFree(h->keys);
      return fail(SPS_ERR_NOMEM, "LTS projection buffers do not fit the device");
    }
    HIP_TRY(hipMemset(h->status, 0, sizeof(int)));
    *out = h.release();
    return SPS_OK;
  }
  if (numel != lts_numel())
    return fail(SPS_ERR_INVALID, "LTS weight blob has %lld floats, expected %lld", (long long)numel, (long long)lts_numel());
  std::map<std::string, const float *> by;
  for (const auto &t : lts_spec()) by[t.name] = blob + t.offset;
  const LtsW L = lts_wlayout();
  std::vector<float> w((size_t)L.total, 0.f);
  // conv (+ bias) followed by BN: rows of W scaled, bias shifted, in f64
  auto fold = [&](const float *W, const float *bias, const std::string &bn, int rows, int k, int64_t wo, int64_t ld,
                  int64_t col0, int64_t wdst, int64_t bdst) {
    const float *g = by[bn + ".weight"], *be = by[bn + ".bias"], *mu = by[bn + ".running_mean"], *var = by[bn + ".running_var"];
    for (int o = 0; o < rows; ++o) {
      const double sc = (double)g[o] / std::sqrt((double)var[o] + 1e-5);
      for (int c = 0; c < k; ++c) w[(size_t)(wdst + (int64_t)o * k + c)] = (float)(W[wo + (int64_t)o * ld + col0 + c] * sc);
      if (bdst >= 0) w[(size_t)(bdst + o)] = (float)(((bias ? (double)bias[o] : 0.0) - mu[o]) * sc + be[o]);
    }
  };
  fold(by["embedding.conv1.weight"], nullptr, "embedding.bn1", 128, 3, 0, 3, 0, L.e1w, L.e1b);
  fold(by["embedding.conv2.weight"], nullptr, "embedding.bn2", 128, 128, 0, 128, 0, L.e2w, L.e2b);
  for (int k = 0; k < 4; ++k) {
    const std::string p = "sa" + std::to_string(k + 1);
    // q_conv.weight IS k_conv.weight (transformer.py:42): loading a state_dict assigns the shared Parameter twice and
    // k_conv, loaded second, wins
    const float *kw = by[p + ".k_conv.weight"], *vw = by[p + ".v_conv.weight"], *vb = by[p + ".v_conv.bias"];
    std::copy(kw, kw + 32 * 128, w.begin() + L.qvw[k]);
    std::copy(vw, vw + 128 * 128, w.begin() + L.qvw[k] + 32 * 128);
    std::copy(vb, vb + 128, w.begin() + L.qvb[k] + 32);
    fold(by[p + ".trans_conv.weight"], by[p + ".trans_conv.bias"], p + ".after_norm", 128, 128, 0, 128, 0, L.tw[k], L.tb[k]);
  }
  fold(by["linear1.0.weight"], nullptr, "linear1.1", 2048, 512, 0, 512, 0, L.l1w, L.l1b);
  const float *w2 = by["linear2.0.weight"];
  fold(w2, by["linear2.0.bias"], "linear2.1", 512, 2048, 0, 6144, 0, L.l2w, L.l2b);
  fold(w2, nullptr, "linear2.1", 512, 4096, 0, 6144, 2048, L.l2p, -1);
  fold(by["linear3.0.weight"], by["linear3.0.bias"], "linear3.1", 256, 512, 0, 512, 0, L.l3w, L.l3b);
  std::copy(by["convs.weight"], by["convs.weight"] + 256, w.begin() + L.hw);

  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<sps_lts> h(new sps_lts);
  h->device = device;
  h->L = L;
  h->head_bias = by["convs.bias"][0];
  if (hipMalloc(&h->w, (size_t)L.total * sizeof(float)) != hipSuccess ||
      hipMalloc(&h->status, sizeof(int)) != hipSuccess ||
      hipMalloc(&h->keys, sizeof(unsigned long long) * 2 * 32 * LTS_SLICES) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(h->w);
    (void)hipFree(h->status);
    (void)hipFree(h->keys);
    return fail(SPS_ERR_NOMEM, "LTS weights do not fit the device");
  }
  HIP_TRY(hipMemcpy(h->w, w.data(), (size_t)L.total * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(h->status, 0, sizeof(int)));
  *out = h.release();
  return SPS_OK;
}

int sps_lts_destroy(sps_lts *h) {
  if (!h) return SPS_OK;
  int prev = -1;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  lts_free_ws(h);
  (void)hipFree(h->w);
  (void)hipFree(h->status);
  (void)hipFree(h->keys);
  if (prev >= 0 && prev != h->device) (void)hipSetDevice(prev);
  delete h;
  return SPS_OK;
}

int sps_lts_project(sps_lts *h, const float *pts_dev, int64_t ld, int64_t n, int lidar, float *frame_dev, float *x_dev,
                    float *rows_dev, void *stream) {
  LtsLidar L;
  if (!h || !frame_dev) return fail(SPS_ERR_INVALID, "null argument");
  if (!lts_lidar(lidar, &L)) return fail(SPS_ERR_INVALID, "lidar must be 0 (vlp-16) or 1 (hdl-32)");
  if (n < 0 || n > SPS_MAX_POINTS || ld < 4 || (n > 0 && !pts_dev)) return fail(SPS_ERR_INVALID, "bad arguments");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const int cells = L.beams * LTS_SLICES;
  unsigned long long *kxy = h->keys, *kzs = h->keys + 32 * LTS_SLICES;
  HIP_TRY(hipMemsetAsync(frame_dev, 0, (size_t)cells * 4 * sizeof(float), st));
  HIP_TRY(hipMemsetAsync(h->keys, 0, sizeof(unsigned long long) * 2 * 32 * LTS_SLICES, st));
  if (n > 0) {
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_lts_proj_xy, dim3(nb), dim3(256), 0, st, pts_dev, ld, (int)n, L, kxy, h->status);
    hipLaunchKernelGGL(k_lts_proj_zs, dim3(nb), dim3(256), 0, st, pts_dev, ld, (int)n, L, (const unsigned long long *)kxy, kzs);
    hipLaunchKernelGGL(k_lts_proj_write, dim3(nb), dim3(256), 0, st, pts_dev, ld, (int)n, L, (const unsigned long long *)kxy,
                       (const unsigned long long *)kzs, frame_dev);
  }
  if (x_dev || rows_dev)
    hipLaunchKernelGGL(k_lts_proj_unpack, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, (const float *)frame_dev, L,
                       x_dev, rows_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int sps_lts_forward(sps_lts *h, const float *x_dev, int64_t B, int64_t N, float *scores_dev, void *stream) {
  if (!h || !x_dev || !scores_dev) return fail(SPS_ERR_INVALID, "null argument");
  if (!h->w) return fail(SPS_ERR_NOWEIGHTS, "this LTS handle was created without weights (projection only)");
  if (B < 1 || N < 1 || B > 65535 || N > (1 << 20) || B * N > SPS_MAX_POINTS)
    return fail(SPS_ERR_INVALID, "bad shape B=%lld N=%lld", (long long)B, (long long)N);
  HIP_TRY(hipSetDevice(h->device));
  int rc = lts_reserve(h, B, N);
  if (rc != SPS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const LtsW &L = h->L;
  const float *w = h->w;
  const int64_t R = B * N;
  const int Bi = (int)B, Ni = (int)N;
  const int mtiles = (Ni + LG_T - 1) / LG_T;

  hipLaunchKernelGGL(k_lts_embed1, dim3((unsigned)((R * 128 + 255) / 256)), dim3(256), 0, st, x_dev, Bi, Ni, w + L.e1w,
                     w + L.e1b, h->d);
  lts_gemm<LE_RELU>(st, Bi, lts_g(h->d, 128, w + L.e2w, w + L.e2b, h->emb, 128, Ni, 128, 128));

  // pass-B splits of the query axis: enough waves to fill the device, in whole 32-row tiles
  const int ktiles = (Ni + 31) / 32;
  int splits = (int)std::min<int64_t>(LTS_MAX_SPLITS, std::max<int64_t>(1, 2048 / (B * ktiles)));
  splits = std::min(splits, ktiles);
  const int rows_per_split = ((ktiles + splits - 1) / splits) * 32;
  splits = (Ni + rows_per_split - 1) / rows_per_split;
  const int64_t split_stride = R * LTS_PL;
  for (int k = 0; k < 4; ++k) {
    const float *xin = k == 0 ? h->emb : h->cat + (k - 1) * 128;
    const int64_t ldx = k == 0 ? 128 : 512;
    lts_gemm<LE_BIAS>(st, Bi, lts_g(xin, ldx, w + L.qvw[k], w + L.qvb[k], h->qv, LTS_QV, Ni, LTS_QV, 128));
    hipLaunchKernelGGL(k_lts_attn_stats, dim3((unsigned)ktiles, (unsigned)B), dim3(64), 0, st, (const float *)h->qv, Ni,
                       h->mrow, h->rl);
    hipLaunchKernelGGL(k_lts_attn_out, dim3((unsigned)ktiles, (unsigned)B, (unsigned)splits), dim3(64), 0, st,
                       (const float *)h->qv, Ni, (const float *)h->mrow, (const float *)h->rl, rows_per_split, h->part,
                       split_stride);
    hipLaunchKernelGGL(k_lts_attn_combine, dim3((unsigned)((R * 128 + 255) / 256)), dim3(256), 0, st, (const float *)h->part,
                       splits, split_stride, R, xin, ldx, h->d);
    LtsGemm g = lts_g(h->d, 128, w + L.tw[k], w + L.tb[k], h->cat + k * 128, 512, Ni, 128, 128);
    g.R = xin;
    g.ldr = ldx;
    lts_gemm<LE_RES_RELU>(st, Bi, g);
  }
  LtsGemm g1 = lts_g(h->cat, 512, w + L.l1w, w + L.l1b, h->y1, 2048, Ni, 2048, 512);
  g1.pmax = h->pmax;
  g1.psum = h->psum;
  g1.mtiles = mtiles;
  lts_gemm<LE_LRELU_POOL>(st, Bi, g1);
  hipLaunchKernelGGL(k_lts_pool, dim3(2048 / 256, (unsigned)B), dim3(256), 0, st, (const float *)h->pmax,
                     (const float *)h->psum, mtiles, 2048, Ni, h->gmax, h->gmean);
  hipLaunchKernelGGL(k_lts_wbias, dim3((unsigned)((B * 512 + 3) / 4)), dim3(256), 0, st, w + L.l2p, w + L.l2b,
                     (const float *)h->gmax, (const float *)h->gmean, Bi, h->wb);
  LtsGemm g2 = lts_g(h->y1, 2048, w + L.l2w, nullptr, h->h2, 512, Ni, 512, 2048);
  g2.wbias = h->wb;
  lts_gemm<LE_SILU_WBIAS>(st, Bi, g2);
  lts_gemm<LE_SILU>(st, Bi, lts_g(h->h2, 512, w + L.l3w, w + L.l3b, h->h3, 256, Ni, 256, 512));
  hipLaunchKernelGGL(k_lts_head, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, (const float *)h->h3, R, w + L.hw,
                     h->head_bias, scores_dev);
  HIP_TRY(hipGetLastError());
  h->last_b = B;
  h->last_n = N;
  return SPS_OK;
}

int sps_lts_check(sps_lts *h, void *stream) {
  if (!h) return fail(SPS_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  int e = 0;
  HIP_TRY(hipMemcpyAsync(&e, h->status, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (e == 0) return SPS_OK;
  HIP_TRY(hipMemsetAsync(h->status, 0, sizeof(int), st));
  HIP_TRY(hipStreamSynchronize(st));
  if (e & 2) return fail(SPS_ERR_RANGE, "IndexError: a point has a NaN coordinate (loader.py:45-53 cannot index it)");
  return fail(SPS_ERR_RANGE, "IndexError: a point's elevation is outside the lidar's image rows (loader.py:51-56)");
}

int sps_lts_tap(sps_lts *h, int which, float *out_dev, int64_t *rows, int64_t *cols, void *stream) {
  if (!h) return fail(SPS_ERR_INVALID, "null handle");
  if (h->last_b == 0) return fail(SPS_ERR_INVALID, "no forward has run on this handle");
  const int64_t R = h->last_b * h->last_n;
  const float *src = nullptr;
  int64_t r = R, c = 128, lds = 128;
  if (which == 0) {
    src = h->emb;
  } else if (which >= 1 && which <= 4) {
    src = h->cat + (which - 1) * 128;
    lds = 512;
  } else if (which == 5 || which == 6) {
    src = which == 5 ? h->gmax : h->gmean;
    r = h->last_b;
    c = lds = 2048;
  } else {
    return fail(SPS_ERR_INVALID, "unknown tap %d (0 embedding, 1-4 sa1-sa4, 5 linear1 max, 6 linear1 mean)", which);
  }
  if (rows) *rows = r;
  if (cols) *cols = c;
  if (!out_dev) return SPS_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpy2DAsync(out_dev, (size_t)c * sizeof(float), src, (size_t)lds * sizeof(float), (size_t)c * sizeof(float),
                           (size_t)r, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SPS_OK;
}
