// train_host.inc.h -- part of sps_hip.hip (included inside its extern "C" block): orchestration of one training step
// of the SPS network on the context's device (reference src/sps/models/models.py:62-82 + :154-160).
//
//   sps_train_forward : quantise / voxelise / maps exactly as sps_forward, then CustomMinkUNet14 in TRAIN mode -- every
//                       conv writes its raw output z, BatchNorm uses the batch statistics of the active rows, the block
//                       wiring (residual, 1x1 downsample branch, concat) is that of minkunet.py:161-219 -- slice, sigmoid.
//                       Saves what the backward needs inside the context.
//   sps_train_backward: d(loss)/d(scores) in, gradient of every parameter out (flat blob in the layout of
//                       sps_weights_tensor_info).  Data gradients reuse the forward's gather kernels over the same
//                       kernel maps with mirrored / transposed weights; weight gradients are MFMA reductions over the
//                       map's pairs (k_wgrad); BN / ReLU / residual backward in k_bn_bwd_*.
// The op list of a step (train_ops) is the wiring table of netspec.inc.h resolved against the training views -- the same
// rows the inference forward walks; conv_plain fills its ConvArgs through conv_args and launches through launch_upconv /
// launch_k_conv, the launchers of the inference path (sps_hip.hip).
// The loss (nn.MSELoss on the scan rows, models.py:62-70) and the optimiser (Adam + StepLR, models.py:154-160) stay in
// torch: they are a handful of elementwise kernels on tensors torch already owns.

extern "C++" {
namespace {

struct TView {      // a feature tensor view: `cols` columns starting at column 0 of (ptr, ld); g = its gradient
  float *p = nullptr, *g = nullptr;
  int ld = 0, cols = 0, level = 0;
};

struct TOp {
  int conv;          // index into NetSpec::convs (its BN: bn_idx)
  ConvKind kind;
  TView in, out;     // out = destination of relu?(bn(z) [+ res])
  int relu;
  TView res;         // residual operand (p == nullptr: none)
};

}  // namespace

struct WgPlan {  // k_wgrad<aw, bw> over (nwg, K, zblocks) workgroups; nwg > 1: partials in slab + slab_off, reduced at the end
  int aw = 1, bw = 1, zblocks = 1, NB = 1, nwg = 1, gshift = 6;
  int64_t slab_off = 0;
};

struct sps_train {
  int64_t cap = 0;
  uint64_t arena_gen = 0;  // generation of the context's arena the views below point into
  const NetSpec *net = nullptr;
  std::vector<void *> allocs;
  float *blob = nullptr, *grad = nullptr;  // parameters / gradients, flat [numel]
  float *wu = nullptr, *wut = nullptr;     // forward / data-gradient MFMA operands
  std::vector<int64_t> wu_off, wut_off;    // per conv (floats)
  std::vector<float *> z;                  // per conv: raw output [cap, cout]
  float *gpool = nullptr;                  // gradients of the feature buffers (one allocation, zeroed per backward)
  size_t gpool_bytes = 0;
  std::vector<float *> r_p, r_g;           // per downsample conv: its BN'd output (the residual operand of the block's conv2)
  std::vector<float *> dzl;                // per conv: gradient wrt its raw output [cap, cout] (kept until the weight gradients run, at the end)
  std::vector<WgradJobs> wjobs;            // weight-gradient jobs of the running backward, by block shape (wgrad_shape_index)
  float *slab = nullptr;                   // workgroup partials of the weight gradients, every layer its own region
  size_t slab_floats = 0;
  std::vector<WgPlan> wg;                  // per conv: geometry of its k_wgrad launch
  double *bn_part = nullptr, *bn_bpart = nullptr, *fin_part = nullptr;
  float *bn_fin = nullptr;                 // per BN [2][BN_MAXC]: mean, invstd
  float *batch_stats = nullptr;            // per BN [2][C] at 2 * ss_off-like offsets (same as c->ss layout)
  float *ones = nullptr, *zeros = nullptr;
  float *c0part = nullptr;
  PermDesc *perm = nullptr;                // operand table of k_permute_weights (one launch per step)
  int n_perm = 0, perm_blocks = 0;
  long long *vacc = nullptr;
  // gradient views of the context's feature buffers, by FeatId
  std::vector<TView> views;
  int64_t n_last = 0;
  bool have_forward = false;
  uint64_t fwd_gen = 0;  // c->fwd_gen of the forward whose activations are held
};

namespace {

void train_free(sps_train *t) {
  for (void *p : t->allocs) (void)hipFree(p);
  t->allocs.clear();
  t->cap = 0;
  t->have_forward = false;
}

constexpr int C0_WG = 1024;  // workgroups (x 4 waves, one row at a time each) of k_conv0_wgrad

#define TALLOC(ptr, type, count)                                                                    \
  do {                                                                                              \
    void *p_ = nullptr;                                                                             \
    hipError_t e_ = hipMalloc(&p_, sizeof(type) * (size_t)((count) > 0 ? (count) : 4));             \
    if (e_ != hipSuccess) return fail(SPS_ERR_NOMEM, "hipMalloc (training arena) failed: %s", hipGetErrorString(e_)); \
    t->allocs.push_back(p_);                                                                        \
    ptr = reinterpret_cast<type *>(p_);                                                             \
  } while (0)

std::vector<TOp> train_ops(sps_ctx *c);
inline bool is_downsample(const TOp &op) { return op.kind == T_LIN; }

int train_reserve(sps_ctx *c) {
  if (!c->train) c->train = new sps_train();
  sps_train *t = c->train;
  if (t->cap == c->cap && t->net == c->net && t->cap > 0 && t->arena_gen == c->arena_gen) return SPS_OK;
  HIP_TRY(hipDeviceSynchronize());
  train_free(t);
  const NetSpec &s = *c->net;
  const int64_t cap = c->cap;
  t->net = &s;
  TALLOC(t->blob, float, s.numel);
  TALLOC(t->grad, float, s.numel);
  // MFMA operands: forward (C_in x C_out) and data gradient (C_out x C_in) per conv
  t->wu_off.assign(s.convs.size(), 0);
  t->wut_off.assign(s.convs.size(), 0);
  int64_t nwu = 0, nwut = 0;
  for (size_t i = 0; i < s.convs.size(); ++i) {
    const ConvSpec &cs = s.convs[i];
    t->wu_off[i] = nwu;
    t->wut_off[i] = nwut;
    if (cs.cin == 1 || (int)i == s.final_idx) continue;
    nwu += (int64_t)cs.K * (cs.cin / 4) * ((cs.cout + 15) / 16) * 64;
    nwut += (int64_t)cs.K * (cs.cout / 4) * ((cs.cin + 15) / 16) * 64;
  }
  TALLOC(t->wu, float, nwu);
  TALLOC(t->wut, float, nwut);
  t->z.assign(s.convs.size(), nullptr);
  for (size_t i = 0; i < s.convs.size(); ++i) {
    if ((int)i == s.final_idx) continue;
    TALLOC(t->z[i], float, (size_t)cap * s.convs[i].cout);
  }
  // gradients of the feature buffers (same shapes) + of the residual operands, one pool
  size_t gfloats = 0, rfloats = 0;
  for (const FeatShape &f : FEAT) gfloats += (size_t)cap * f.ld;
  for (const ConvSpec &cs : s.convs)
    if (cs.ds_idx >= 0) rfloats += (size_t)cap * cs.cout;
  TALLOC(t->gpool, float, gfloats + rfloats);
  t->gpool_bytes = (gfloats + rfloats) * sizeof(float);
  t->views.clear();
  float *gp = t->gpool;
  for (int f = 0; f < N_FEAT; ++f) {
    t->views.push_back(TView{c->feat[f], gp, FEAT[f].ld, FEAT[f].ld, FEAT[f].level});
    gp += (size_t)cap * FEAT[f].ld;
  }
  t->r_p.assign(s.convs.size(), nullptr);
  t->r_g.assign(s.convs.size(), nullptr);
  for (const ConvSpec &cs : s.convs) {  // (in block order)
    if (cs.ds_idx < 0) continue;
    t->r_g[cs.ds_idx] = gp;
    gp += (size_t)cap * cs.cout;
    TALLOC(t->r_p[cs.ds_idx], float, (size_t)cap * cs.cout);
  }
  t->dzl.assign(s.convs.size(), nullptr);
  for (size_t i = 0; i < s.convs.size(); ++i) {
    if ((int)i == s.final_idx) continue;
    TALLOC(t->dzl[i], float, (size_t)cap * s.convs[i].cout);
  }
  // weight gradients: a wave owns aw x bw tiles of 16 x 16 of dW[k] and one chunk of the level's row tiles; the rows are cut
  // into nwg x 16 chunks so that ~16 k waves exist whatever the layer's K x block count (every wave walks its chunk as a
  // chain of dependent loads: short chunks also bound the launch's duration), with at least ~128 rows per chunk at the row
  // count a level typically has (a prior: the real count is only known on the device; it does not affect results beyond
  // the summation order, which stays fixed for a given capacity)
  {
    // (tests/train_edge_inputs.py::plan restates this block to choose capacities; the GPU edge tests read the result back
    // through sps_train_wgrad_plan and fail if the two part)
    static const double level_prior[SPS_NUM_LEVELS] = {1.0, 0.5, 0.2, 0.06, 0.02};
    int64_t wave_target = 16384;  // waves a weight-gradient launch aims for (8 k: +15 us, 32 k: -5 us on the level-0 layers, +8 % on the coarse ones)
#if defined(SPS_DIAG)
    if (const char *wenv = getenv("SPS_WGRAD_WAVES"))
      if (atoi(wenv) > 0) wave_target = atoi(wenv);
#endif
    t->wg.assign(s.convs.size(), WgPlan{});
    int64_t off = 0;
    for (const TOp &op : train_ops(c)) {
      if (op.kind == T_CONV0) continue;
      const int i = op.conv;
      const ConvSpec &cs = s.convs[i];
      const int level = op.kind == T_UP ? op.out.level + 1 : op.out.level;  // the level whose rows the map lists
      WgPlan &w = t->wg[i];
      w.aw = cs.cin >= 24 ? 2 : 1;
      w.bw = cs.cout >= 64 ? 4 : cs.cout >= 32 ? 2 : 1;
      w.NB = (cs.cout + 16 * w.bw - 1) / (16 * w.bw);
      w.zblocks = ((cs.cin + 16 * w.aw - 1) / (16 * w.aw)) * w.NB;
      const int64_t tiles = std::max<int64_t>(64, (int64_t)(level_prior[level] * (double)cap) / 16);
      // rows are read 64 at a time, 16 where pairs of 64-row groups would not make ~4 k waves (1x1 maps, coarse stride maps)
      w.gshift = (int64_t)cs.K * w.zblocks * (tiles / 8) < 4096 ? 4 : 6;
      const int64_t groups = w.gshift == 4 ? tiles : tiles / 4;
      const int64_t want = std::min<int64_t>(1024, std::max<int64_t>(WG_WAVES, wave_target / ((int64_t)cs.K * w.zblocks)));
      int nwg = (int)((want + WG_WAVES - 1) / WG_WAVES);
      while (nwg > 1 && (int64_t)nwg * WG_WAVES * (w.gshift == 4 ? 4 : 2) > groups) nwg >>= 1;
      w.nwg = nwg;
      w.slab_off = off;
      if (nwg > 1) off += (int64_t)nwg * cs.K * cs.cin * cs.cout;
    }
    t->slab_floats = (size_t)off;
    TALLOC(t->slab, float, t->slab_floats);
  }
  TALLOC(t->bn_part, double, (size_t)s.bns.size() * BN_WG * 2 * BN_MAXC);
  TALLOC(t->bn_bpart, double, (size_t)2 * BN_WG * 2 * BN_MAXC);
  TALLOC(t->fin_part, double, (size_t)BN_WG * 9);
  for (const BnSpec &b : s.bns)
    if (b.c < 8 || b.c > BN_MAXC || (b.c & (b.c - 1)))
      return fail(SPS_ERR_INVALID, "training BatchNorm kernels need 8 <= C <= %d, a power of two (got %d)", BN_MAXC, b.c);
  TALLOC(t->bn_fin, float, (size_t)s.bns.size() * 2 * BN_MAXC);
  TALLOC(t->batch_stats, float, s.ss_numel / 2 * 3);
  TALLOC(t->ones, float, 128);
  TALLOC(t->zeros, float, 128);
  TALLOC(t->c0part, float, (size_t)C0_WG * 1000);
  {
    std::vector<PermDesc> pd;
    int blk = 0;
    for (size_t i = 0; i < s.convs.size(); ++i) {
      const ConvSpec &cs = s.convs[i];
      if (cs.cin == 1 || (int)i == s.final_idx) continue;
      // forward operand, then the data-gradient operand: symmetric 3^4 maps mirror the offset; stride / transposed / 1x1 maps keep it
      const int modes[2] = {0, cs.K == 81 ? 1 : 2};
      for (int mode : modes) {
        const int tot = mode == 0 ? cs.K * (cs.cin / 4) * ((cs.cout + 15) / 16) * 64 : cs.K * (cs.cout / 4) * ((cs.cin + 15) / 16) * 64;
        PermDesc d{};
        d.w_off = cs.w_off;
        d.dst_off = mode == 0 ? t->wu_off[i] : t->wut_off[i];
        d.K = cs.K, d.cin = cs.cin, d.cout = cs.cout, d.mode = mode;
        d.blk0 = blk;
        d.nblk = std::min(64, (tot + 255) / 256);
        blk += d.nblk;
        pd.push_back(d);
      }
    }
    t->n_perm = (int)pd.size();
    t->perm_blocks = blk;
    TALLOC(t->perm, PermDesc, pd.size());
    HIP_TRY(hipMemcpy(t->perm, pd.data(), pd.size() * sizeof(PermDesc), hipMemcpyHostToDevice));
  }
  TALLOC(t->vacc, long long, cap);
  std::vector<float> one(128, 1.f);
  HIP_TRY(hipMemcpy(t->ones, one.data(), 128 * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(t->zeros, 0, 128 * sizeof(float)));
  HIP_TRY(hipMemset(t->batch_stats, 0, s.ss_numel / 2 * 3 * sizeof(float)));
  t->cap = cap;
  t->arena_gen = c->arena_gen;
  return SPS_OK;
}

inline bool vec4_ok(const float *p, int ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0; }

TView cols_of(TView v, int col0, int cols) {  // sub-view: columns [col0, col0 + cols)
  v.p += col0;
  v.g += col0;
  v.cols = cols;
  return v;
}

// the network as a list of conv + BN (+ residual) (+ ReLU) ops in forward order: the rows of the wiring table (netspec.inc.h)
// resolved against the training views, plus, before conv2 of a block with a downsample, the T_LIN op that writes the BN'd
// 1x1 branch of the block input into its own buffer -- conv2's residual operand (resnet BasicBlock)
std::vector<TOp> train_ops(sps_ctx *c) {
  sps_train *t = c->train;
  const NetSpec &s = *t->net;
  auto V = [&](FeatView v) { return v.buf < 0 ? TView{} : cols_of(t->views[v.buf], v.col0, v.cols); };
  std::vector<TOp> ops;
  for (const LayerRow &r : s.layers) {
    const ConvSpec &cs = s.convs[r.conv];
    TView res = V(r.blk);
    if (cs.ds_idx >= 0) {
      res = TView{t->r_p[cs.ds_idx], t->r_g[cs.ds_idx], cs.cout, cs.cout, r.level};
      ops.push_back({cs.ds_idx, T_LIN, V(r.blk), res, 0, TView{}});
    }
    ops.push_back({r.conv, r.kind, V(r.in), V(r.out), r.relu, res});
  }
  return ops;
}

// A plain sparse convolution launch (no BN / residual / fusion): out[o][:] (= or +=) sum_k in[map_k(o)] W'[k], through
// k_conv (gather maps: 3^4 tables, `down` tables, identity) or k_upconv (parent-stationary over a `down` table).
//   gather : T_K3 (nbr3 of level_rows), T_DOWN (down table of level_rows: rows = coarse), T_LIN (identity), or
//            T_UP (k_upconv: rows iterate the COARSE level level_rows, children written at the fine level)
int conv_plain(sps_ctx *c, hipStream_t st, ConvKind gather, int level_rows, int K, int cin, int cout, const float *Wu,
               const float *in, int ldi, float *out, int ldo, bool accumulate) {
  sps_train *t = c->train;
  ConvArgs a = conv_args(c, level_rows, K, cin, cout, Wu, t->ones, t->zeros, in, ldi, out, ldo, accumulate ? out : nullptr, ldo);
  a.in_bytes = (uint32_t)((size_t)c->cap * (size_t)ldi * 4u);  // training runs on dense arenas: every level holds cap rows
  a.wu_bytes = (uint32_t)((size_t)K * a.upk * a.NT * 64 * 4);
  const Map map = level_map(c, gather, level_rows);  // T_LIN: identity (nbr = tmask = null)
  a.nbr = map.nbr;
  a.tmask = map.tmask;
  if (gather == T_UP) return launch_upconv(a, c->cap, level_rows, st);
  // the inference geometry of the level (column tiles per wave x splits); NT = 3 / 6 (gradients wrt 48 / 96 channels)
  // only divide by one column tile per wave
  Geometry g = conv_geometry(level_rows, K, cin, a.NT);
  if (a.NT % g.ntw != 0) g.ntw = 1;
  a.S = g.S;
  const dim3 grid((unsigned)(a.NT / g.ntw), (unsigned)(row_grid(c->cap, level_rows) * g.S), 1u);
  return launch_k_conv(a, g, false, grid, st);
}

constexpr int WGRAD_SHAPES = 6;
inline int wgrad_shape_index(int aw, int bw) {  // <1,1> <1,2> <1,4> <2,1> <2,2> <2,4>
  return (aw == 2 ? 3 : 0) + (bw == 4 ? 2 : bw == 2 ? 1 : 0);
}

// The weight gradient of a layer joins the job table of its block shape; wgrad_run launches the tables at the end of the backward.
int wgrad_defer(sps_ctx *c, ConvKind kind, int conv_index, int level_rows, int K, int cin, int cout, const float *x, int ldx,
                const float *dz, int ldz, float *dW) {
  sps_train *t = c->train;
  const WgPlan &pl = t->wg[conv_index];
  WgradArgs w{};
  w.x = x;
  w.ldx = ldx;
  w.dz = dz;
  w.ldz = ldz;
  w.K = K;
  w.cin = cin;
  w.cout = cout;
  w.NB = pl.NB;
  w.gshift = pl.gshift;
  // extents for the raw buffer loads (training runs on dense arenas: every level's buffers hold cap rows)
  w.x_bytes = (uint32_t)((size_t)c->cap * (size_t)ldx * 4u);
  w.dz_bytes = (uint32_t)((size_t)c->cap * (size_t)ldz * 4u);
  w.ldn = c->capl[level_rows];
  w.n_rows = c->counts + level_rows;
  w.gather_b = kind == T_UP ? 1 : 0;
  const Map map = level_map(c, kind, level_rows);
  w.nbr = map.nbr;
  w.tmask = map.tmask;
  if ((cin & 7) || (cout & 7) || (ldx & 3) || (ldz & 3) || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(dz) & 15))
    return fail(SPS_ERR_INVALID, "wgrad: operands must be 16-byte aligned with channel counts in multiples of 8");
  w.out = pl.nwg > 1 ? t->slab + pl.slab_off : dW;
  if (!((pl.aw == 1 || pl.aw == 2) && (pl.bw == 1 || pl.bw == 2 || pl.bw == 4)))
    return fail(SPS_ERR_INVALID, "wgrad: no instantiation for a %d x %d block", pl.aw, pl.bw);
  WgradJobs &js = t->wjobs[wgrad_shape_index(pl.aw, pl.bw)];
  if (js.n >= WG_MAXJ) return fail(SPS_ERR_INVALID, "wgrad: more than %d layers of one block shape", WG_MAXJ);
  WgradJob &j = js.j[js.n++];
  j.a = w;
  j.nwg = pl.nwg;
  j.wg0 = js.total;
  js.total += pl.nwg * K * pl.zblocks;
  return SPS_OK;
}

template <int AW, int BW>
void wgrad_go(const WgradJobs &js, hipStream_t st) {
  if (js.n) hipLaunchKernelGGL((k_wgrad<AW, BW>), dim3((unsigned)js.total), dim3(WG_WAVES * 64), 0, st, js);
}
void wgrad_run(sps_ctx *c, hipStream_t st) {
  sps_train *t = c->train;
  // the widest blocks first: their workgroups are the longest
  wgrad_go<2, 4>(t->wjobs[5], st);
  wgrad_go<2, 2>(t->wjobs[4], st);
  wgrad_go<1, 4>(t->wjobs[2], st);
  wgrad_go<2, 1>(t->wjobs[3], st);
  wgrad_go<1, 2>(t->wjobs[1], st);
  wgrad_go<1, 1>(t->wjobs[0], st);
}

// the one reduce launch of a backward: every layer whose k_wgrad ran with more than one workgroup per (k, block)
int wgrad_reduce_all(sps_ctx *c, hipStream_t st) {
  sps_train *t = c->train;
  const NetSpec &s = *t->net;
  WRedArgs r{};
  int blk = 0;
  for (size_t i = 0; i < s.convs.size(); ++i) {
    const WgPlan &pl = t->wg[i];
    if (pl.nwg <= 1) continue;
    if (r.n >= WRED_MAX) return fail(SPS_ERR_INVALID, "wgrad: more than %d layers to reduce", WRED_MAX);
    const ConvSpec &cs = s.convs[i];
    WRedDesc &d = r.d[r.n++];
    d.slab_off = pl.slab_off;
    d.w_off = cs.w_off;
    d.total = cs.K * cs.cin * cs.cout;
    d.nwg = pl.nwg;
    d.blk0 = blk;
    d.nblk = std::min(256, (d.total + 255) / 256);
    blk += d.nblk;
  }
  if (r.n) hipLaunchKernelGGL(k_wgrad_reduce_all, dim3((unsigned)blk), dim3(256), 0, st, r, t->slab, t->grad);
  return SPS_OK;
}

}  // namespace
}  // extern "C++"

int sps_train_forward(sps_ctx *c, const float *params_dev, int64_t numel, const float *coords, int64_t ld, int64_t n, float vs,
                      float *scores, float *batch_stats_dev, void *stream) {
  if (!c || !params_dev || !coords || !scores || n <= 0) return fail(SPS_ERR_INVALID, "bad arguments");
  const NetSpec &s = spec(1);
  if (numel != s.numel) return fail(SPS_ERR_INVALID, "parameter blob has %lld floats, expected %lld", (long long)numel, (long long)s.numel);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  if (c->compact) {  // the backward indexes every level's arrays on the host's assumption that nothing was aborted
    c->compact = false;
    if (c->cap > 0) c->regrow = true;
  }
  if (c->lean) {  // the training convolutions and weight gradients read the neighbour tables of every level
    c->lean = false;
    if (c->cap > 0) c->regrow = true;
  }
  // coordinate structures: the inference front-end with the network skipped (weights are not needed for it)
  {
    ForwardOpts fo;
    fo.front_only = true;
    const NetSpec *saved_net = c->net;
    const bool saved_have = c->have_weights;
    c->net = &s;
    c->have_weights = true;
    int rc = forward_impl(c, coords, ld, n, vs, scores, fo, stream);
    c->net = saved_net;
    c->have_weights = saved_have;
    if (rc != SPS_OK) return rc;
  }
  const NetSpec *saved_net = c->net;
  c->net = &s;
  int rc = train_reserve(c);
  c->net = saved_net;
  if (rc != SPS_OK) return rc;
  sps_train *t = c->train;
  t->have_forward = false;
  hipLaunchKernelGGL(k_train_check_rows, dim3(1), dim3(64), 0, st, c->counts, c->err);
  HIP_TRY(hipMemcpyAsync(t->blob, params_dev, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, st));
  // operands of this step's weights
  hipLaunchKernelGGL(k_permute_weights, dim3((unsigned)t->perm_blocks), dim3(256), 0, st, t->perm, t->n_perm, t->blob, t->wu, t->wut);
  const auto ops = train_ops(c);
  // conv1 and the 1x1 downsample of a residual block (consecutive in the list) read the same input: both convolutions are
  // launched, then ONE statistics and ONE apply launch normalise both outputs (blockIdx.y)
  for (size_t oi = 0; oi < ops.size();) {
    const size_t npair = (oi + 1 < ops.size() && is_downsample(ops[oi + 1])) ? 2 : 1;
    BnFwd2 jobs{};
    int64_t apply_items = 0;
    for (size_t j = 0; j < npair; ++j) {
      const TOp &op = ops[oi + j];
      const int ci = op.conv;
      const ConvSpec &cs = s.convs[ci];
      const int bi = cs.bn_idx;
      const BnSpec &bn = s.bns[bi];
      const int lo = op.out.level;
      float *z = t->z[ci];
      if (op.kind == T_CONV0) {
        const int g0 = grid_for(c->cap, 64, 4096);
        hipLaunchKernelGGL(k_conv0_fused, dim3((unsigned)g0), dim3(256), 0, st, c->counts + 0, c->lv[0].view(),
                           t->blob + cs.w_off, t->ones, t->zeros, 0.5f, z, 8, 0, TileOrderArgs{}, g0);
      } else if (op.kind == T_UP) {
        rc = conv_plain(c, st, T_UP, lo + 1, cs.K, cs.cin, cs.cout, t->wu + t->wu_off[ci], op.in.p, op.in.ld, z, cs.cout, false);
      } else {
        rc = conv_plain(c, st, op.kind, lo, cs.K, cs.cin, cs.cout, t->wu + t->wu_off[ci], op.in.p, op.in.ld, z, cs.cout, false);
      }
      if (rc != SPS_OK) return rc;
      if (!vec4_ok(z, cs.cout) || !vec4_ok(op.out.p, op.out.ld) || (op.res.p && !vec4_ok(op.res.p, op.res.ld)))
        return fail(SPS_ERR_INVALID, "training BatchNorm operands must be 16-byte aligned (%s)", cs.name.c_str());
      BnFwd &b = jobs.j[j];
      b.Z = z;
      b.ldz = cs.cout;
      b.Y = op.out.p;
      b.ldy = op.out.ld;
      b.res = op.res.p;
      b.ldr = op.res.ld;
      b.gamma = t->blob + bn.off;
      b.beta = b.gamma + bn.c;
      b.part = t->bn_part + (size_t)bi * BN_WG * 2 * BN_MAXC;
      b.fin = t->bn_fin + (size_t)bi * 2 * BN_MAXC;
      b.batch_stats = t->batch_stats + cs.ss_off / 2 * 3;
      b.n_rows = c->counts + lo;
      b.C = cs.cout;
      b.relu = op.relu;
      apply_items = std::max<int64_t>(apply_items, (c->cap >> lo) * (cs.cout / 4));
    }
    hipLaunchKernelGGL(k_bn_stats, dim3(BN_WG, (unsigned)npair), dim3(BN_TPB), 0, st, jobs);
    // (every workgroup combines the partials itself: no finish launch in between)
    hipLaunchKernelGGL(k_bn_apply, dim3((unsigned)grid_for(apply_items, 256, 1024), (unsigned)npair), dim3(256), 0, st, jobs);
    oi += npair;
  }
  // final 1x1 conv + bias, slice, sigmoid (models.py:28-29)
  const ConvSpec &fs = s.convs[s.final_idx];
  hipLaunchKernelGGL(k_slice_head, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c->feat[F_B8O], FEAT[F_B8O].ld, c->lv[0].inv, (int)n,
                     t->blob + fs.w_off, t->blob + s.bias_off, 1, 1, scores, (int64_t)1, (const int *)nullptr,
                     (const int *)nullptr);
  if (batch_stats_dev)
    HIP_TRY(hipMemcpyAsync(batch_stats_dev, t->batch_stats, (size_t)s.ss_numel / 2 * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
  // the block hashes go back to "free" (the inference forward does this in its tail kernel)
  {
    const PyramidArgs pa = pyramid_args(c);
    const int gbc = grid_for(c->cap >> 2, 256, 256);
    hipLaunchKernelGGL(k_bhash_cleanup, dim3(gbc * NLV), dim3(256), 0, st, pa, gbc);
    c->tables_dirty = false;
  }
  HIP_TRY(hipGetLastError());
  t->n_last = n;
  t->have_forward = true;
  t->fwd_gen = c->fwd_gen;
  return SPS_OK;
}

int sps_train_generation(sps_ctx *c, int64_t *generation) {
  if (!c || !generation) return fail(SPS_ERR_INVALID, "null argument");
  if (!c->train || !c->train->have_forward) return fail(SPS_ERR_INVALID, "sps_train_forward has not been called on this context");
  *generation = (int64_t)c->train->fwd_gen;
  return SPS_OK;
}

int sps_train_wgrad_plan(sps_ctx *c, const char *conv_name, int32_t *gshift, int32_t *nwg) {
  if (!c || !conv_name || !gshift || !nwg) return fail(SPS_ERR_INVALID, "null argument");
  const sps_train *t = c->train;
  if (!t || !t->net || t->cap <= 0) return fail(SPS_ERR_INVALID, "sps_train_forward has not been called on this context");
  const NetSpec &s = *t->net;
  for (size_t i = 0; i < s.convs.size(); ++i) {
    if (s.convs[i].name != conv_name) continue;
    if (s.convs[i].cin == 1 || (int)i == s.final_idx) break;  // conv0 and final have kernels of their own
    *gshift = t->wg[i].gshift;
    *nwg = t->wg[i].nwg;
    return SPS_OK;
  }
  return fail(SPS_ERR_INVALID, "no k_wgrad job for a convolution named '%s'", conv_name);
}

static int train_backward_impl(sps_ctx *c, const float *dscores, const float *scores, float *grad_dev, int64_t numel, void *stream);

int sps_train_backward_at(sps_ctx *c, int64_t generation, const float *dscores, const float *scores, float *grad_dev, int64_t numel,
                          void *stream) {
  if (!c) return fail(SPS_ERR_INVALID, "null argument");
  sps_train *t = c->train;
  if (!t || !t->have_forward) return fail(SPS_ERR_INVALID, "sps_train_forward has not been called on this context");
  if ((uint64_t)generation != t->fwd_gen || c->fwd_gen != t->fwd_gen)
    return fail(SPS_ERR_INVALID, "the activations of that training forward (generation %lld) were overwritten by a later forward on "
                                 "this context (now at %llu): run forward and backward of a step back to back, or use one context "
                                 "per live autograd graph", (long long)generation, (unsigned long long)c->fwd_gen);
  return train_backward_impl(c, dscores, scores, grad_dev, numel, stream);
}

int sps_train_backward(sps_ctx *c, const float *dscores, const float *scores, float *grad_dev, int64_t numel, void *stream) {
  if (!c) return fail(SPS_ERR_INVALID, "null argument");
  if (!c->train || !c->train->have_forward) return fail(SPS_ERR_INVALID, "sps_train_forward has not been called on this context");
  return sps_train_backward_at(c, (int64_t)c->train->fwd_gen, dscores, scores, grad_dev, numel, stream);
}

static int train_backward_impl(sps_ctx *c, const float *dscores, const float *scores, float *grad_dev, int64_t numel, void *stream) {
  if (!c || !dscores || !scores || !grad_dev) return fail(SPS_ERR_INVALID, "null argument");
  sps_train *t = c->train;
  if (!t || !t->have_forward) return fail(SPS_ERR_INVALID, "sps_train_forward has not been called on this context");
  const NetSpec &s = *t->net;
  if (numel != s.numel) return fail(SPS_ERR_INVALID, "gradient blob has %lld floats, expected %lld", (long long)numel, (long long)s.numel);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = t->n_last;
  {  // gradients this backward accumulates into: the rows each level has, the parameter gradients, the logit accumulator
    ZeroArgs z{};
    int nz = 0;
    auto add = [&](float *p, int64_t floats, int level) {
      if (nz < ZERO_MAX) z.d[nz] = ZeroDesc{p, floats, level};
      ++nz;
    };
    for (const TView &v : t->views) add(v.g, v.ld, v.level);
    for (const LayerRow &r : s.layers)
      if (s.convs[r.conv].ds_idx >= 0) add(t->r_g[s.convs[r.conv].ds_idx], s.convs[r.conv].cout, r.level);
    add(t->grad, (numel + 3) & ~(int64_t)3, -1);  // (allocations are padded to 16 bytes)
    add(reinterpret_cast<float *>(t->vacc), 2 * c->cap, -1);
    if (nz > ZERO_MAX) return fail(SPS_ERR_INVALID, "backward: %d buffers to clear, table holds %d", nz, ZERO_MAX);
    hipLaunchKernelGGL(k_zero_grads, dim3(96, (unsigned)nz), dim3(256), 0, st, z, c->counts, c->cap);
  }
  t->wjobs.assign(WGRAD_SHAPES, WgradJobs{});
  // head: sigmoid + slice + final
  const ConvSpec &fs = s.convs[s.final_idx];
  const TView b8o = t->views[F_B8O];
  hipLaunchKernelGGL(k_dlogit_accum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dscores, scores, c->lv[0].inv, (int)n, t->vacc,
                     c->err);
  hipLaunchKernelGGL(k_final_bwd, dim3(BN_WG), dim3(256), 0, st, t->vacc, c->counts + 0, b8o.p, b8o.ld, t->blob + fs.w_off, b8o.g,
                     b8o.ld, t->fin_part);
  hipLaunchKernelGGL(k_final_bwd_reduce, dim3(1), dim3(64), 0, st, t->fin_part, t->grad + fs.w_off, t->grad + s.bias_off);
  const auto ops = train_ops(c);
  // reverse order; the downsample / conv1 pair of a block shares its two BN launches (their gradients are both complete
  // once conv2's have been propagated), then each runs its weight and data gradient (downsample first, as before)
  for (int oi = (int)ops.size() - 1; oi >= 0;) {
    const int npair = (is_downsample(ops[oi]) && oi >= 1) ? 2 : 1;
    BnBwd2 jobs{};
    int64_t apply_items = 0;
    for (int j = 0; j < npair; ++j) {
      const TOp &op = ops[oi - j];
      const int ci = op.conv;
      const ConvSpec &cs = s.convs[ci];
      const int bi = cs.bn_idx;
      const BnSpec &bn = s.bns[bi];
      const int lo = op.out.level;
      if (!vec4_ok(op.out.g, op.out.ld) || (op.res.g && !vec4_ok(op.res.g, op.res.ld)))
        return fail(SPS_ERR_INVALID, "training BatchNorm gradients must be 16-byte aligned (%s)", cs.name.c_str());
      // BN (+ ReLU, + residual) backward: dY -> dZ, dgamma, dbeta, and dA added to the residual operand's gradient
      BnBwd &b = jobs.j[j];
      b.dY = op.out.g;
      b.ldg = op.out.ld;
      b.Y = op.out.p;
      b.ldy = op.out.ld;
      b.Z = t->z[ci];
      b.ldz = cs.cout;
      b.fin = t->bn_fin + (size_t)bi * 2 * BN_MAXC;
      b.gamma = t->blob + bn.off;
      b.bpart = t->bn_bpart + (size_t)j * BN_WG * 2 * BN_MAXC;
      b.dgamma = t->grad + bn.off;
      b.dbeta = t->grad + bn.off + bn.c;
      b.dZ = t->dzl[ci];
      b.lddz = cs.cout;
      b.dres = op.res.g;
      b.lddr = op.res.ld;
      b.n_rows = c->counts + lo;
      b.C = cs.cout;
      b.relu = op.relu;
      apply_items = std::max<int64_t>(apply_items, (c->cap >> lo) * (cs.cout / 4));
    }
    hipLaunchKernelGGL(k_bn_bwd_stats, dim3(BN_WG, (unsigned)npair), dim3(BN_TPB), 0, st, jobs);
    hipLaunchKernelGGL(k_bn_bwd_apply, dim3((unsigned)grid_for(apply_items, 256, 1024), (unsigned)npair), dim3(256), 0, st, jobs);
    for (int j = 0; j < npair; ++j) {
      const TOp &op = ops[oi - j];
      const int ci = op.conv;
      const ConvSpec &cs = s.convs[ci];
      const int lo = op.out.level;
      const float *dz = t->dzl[ci];
      int rc = SPS_OK;
      if (op.kind == T_CONV0) {
        hipLaunchKernelGGL(k_conv0_wgrad, dim3(C0_WG), dim3(256), 0, st, c->counts + 0, c->lv[0].view(), dz, 8, 0.5f, t->c0part);
        hipLaunchKernelGGL(k_conv0_wgrad_reduce, dim3(125), dim3(256), 0, st, t->c0part, C0_WG, t->grad + cs.w_off);
        continue;  // the input feature is a constant: no data gradient
      }
      // weight gradient: pairs of the op's map; data gradient: the transposed map with transposed weights, accumulated
      if (op.kind == T_UP) {
        rc = wgrad_defer(c, T_UP, ci, lo + 1, cs.K, cs.cin, cs.cout, op.in.p, op.in.ld, dz, cs.cout, t->grad + cs.w_off);
        if (rc != SPS_OK) return rc;
        // y[child] = x[parent] W[oct]  =>  dx[parent] += sum over children dy[child] W[oct]^T : a gather over the `down` table
        rc = conv_plain(c, st, T_DOWN, lo + 1, cs.K, cs.cout, cs.cin, t->wut + t->wut_off[ci], dz, cs.cout, op.in.g, op.in.ld, true);
      } else if (op.kind == T_DOWN) {
        rc = wgrad_defer(c, T_DOWN, ci, lo, cs.K, cs.cin, cs.cout, op.in.p, op.in.ld, dz, cs.cout, t->grad + cs.w_off);
        if (rc != SPS_OK) return rc;
        // z[parent] = sum over children x[child] W[oct]  =>  dx[child] += dz[parent] W[oct]^T : parent-stationary scatter
        rc = conv_plain(c, st, T_UP, lo, cs.K, cs.cout, cs.cin, t->wut + t->wut_off[ci], dz, cs.cout, op.in.g, op.in.ld, true);
      } else {
        rc = wgrad_defer(c, op.kind, ci, lo, cs.K, cs.cin, cs.cout, op.in.p, op.in.ld, dz, cs.cout, t->grad + cs.w_off);
        if (rc != SPS_OK) return rc;
        rc = conv_plain(c, st, op.kind, lo, cs.K, cs.cout, cs.cin, t->wut + t->wut_off[ci], dz, cs.cout, op.in.g, op.in.ld, true);
      }
      if (rc != SPS_OK) return rc;
    }
    oi -= npair;
  }
  wgrad_run(c, st);
  {
    const int rc = wgrad_reduce_all(c, st);
    if (rc != SPS_OK) return rc;
  }
  HIP_TRY(hipMemcpyAsync(grad_dev, t->grad, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int sps_scan_mse(const float *scores_dev, const float *labels_dev, int64_t ld_labels, const float *t_dev, int64_t ld_t, int64_t n,
                 double *work_dev, float *out_dev, void *stream) {
  if (!scores_dev || !labels_dev || !t_dev || !work_dev || !out_dev || n < 0 || n > SPS_MAX_POINTS)
    return fail(SPS_ERR_INVALID, "sps_scan_mse: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mse_partial, dim3(MSE_WG), dim3(256), 0, st, scores_dev, labels_dev, ld_labels, t_dev, ld_t, (int)n, work_dev);
  hipLaunchKernelGGL(k_mse_finish, dim3(1), dim3(64), 0, st, work_dev, out_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}

int sps_scan_mse_backward(const float *scores_dev, const float *labels_dev, int64_t ld_labels, const float *t_dev, int64_t ld_t,
                          int64_t n, const double *work_dev, const float *gloss_dev, float *dscores_dev, void *stream) {
  if (!scores_dev || !labels_dev || !t_dev || !work_dev || !gloss_dev || !dscores_dev || n < 0 || n > SPS_MAX_POINTS)
    return fail(SPS_ERR_INVALID, "sps_scan_mse_backward: bad arguments");
  if (n == 0) return SPS_OK;
  hipLaunchKernelGGL(k_mse_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scores_dev, labels_dev,
                     ld_labels, t_dev, ld_t, (int)n, work_dev, gloss_dev, dscores_dev);
  HIP_TRY(hipGetLastError());
  return SPS_OK;
}
