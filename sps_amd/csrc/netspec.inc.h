// netspec.inc.h -- part of the single translation unit sps_hip.hip (included inside its anonymous namespace).
// CustomMinkUNet14 in one place: the feature buffers (FeatId / FEAT), the layer / parameter inventory with the weight-blob
// layout (ConvSpec, BnSpec), and the wiring table (LayerRow) that the inference forward, the training step and the feature
// taps all read.  build_spec generates convolutions and rows in the same loops and check_wiring cross-checks them once.

// ------------------------------------------------------------------------------------------
// network description (CustomMinkUNet = MinkUNet14 wiring, customminkunet.py:10-12)
// ------------------------------------------------------------------------------------------
constexpr int PLANES[8] = {8, 16, 32, 64, 64, 32, 16, 8};
constexpr int INIT_DIM = 8;

// The context's feature buffers: row-major f32 [rows of `level`, ld].  The order is the allocation order of the arena and
// of the training gradients' pool.  catN is the input of decoder block N: [convtr(N-1) output | encoder skip] (ME.cat is
// a column offset); xN the stride-2 conv into level N; bNt / bNo the conv1 / conv2 output of block N.
enum FeatId { F_CAT8, F_B8T, F_B8O, F_X1, F_B1T, F_CAT7, F_B7T, F_B7O, F_X2, F_B2T, F_CAT6, F_B6T, F_B6O, F_X3, F_B3T,
              F_CAT5, F_B5T, F_B5O, F_X4, F_B4T, F_B4O, N_FEAT };
struct FeatShape {
  int ld, level;
};
constexpr FeatShape FEAT[N_FEAT] = {{16, 0}, {8, 0},  {8, 0},  {8, 1},  {8, 1},  {24, 1}, {16, 1}, {16, 1}, {8, 2},  {16, 2}, {48, 2},
                                    {32, 2}, {32, 2}, {16, 3}, {32, 3}, {96, 3}, {64, 3}, {64, 3}, {32, 4}, {64, 4}, {64, 4}};
struct FeatView {  // columns [col0, col0 + cols) of a feature buffer (buf < 0: none)
  int buf = -1, col0 = 0, cols = 0;
};
constexpr FeatView whole(int buf) { return FeatView{buf, 0, FEAT[buf].ld}; }
constexpr int F_X[4] = {F_X1, F_X2, F_X3, F_X4};
constexpr int F_BT[8] = {F_B1T, F_B2T, F_B3T, F_B4T, F_B5T, F_B6T, F_B7T, F_B8T};
constexpr int F_BO[5] = {F_B4O, F_B5O, F_B6O, F_B7O, F_B8O};  // blocks 1-3 write into the decoder's concat buffers
constexpr int F_CAT[4] = {F_CAT5, F_CAT6, F_CAT7, F_CAT8};    // by decoder stage

// what sps_get_feature hands out
struct FeatTap {
  const char *name;
  FeatView v;
};
constexpr FeatTap FEATURE_TAPS[9] = {
    {"out_p1", {F_CAT8, 8, 8}},   {"block1", {F_CAT7, 16, 8}}, {"block2", {F_CAT6, 32, 16}},
    {"block3", {F_CAT5, 64, 32}}, {"block4", whole(F_B4O)},    {"block5", whole(F_B5O)},
    {"block6", whole(F_B6O)},     {"block7", whole(F_B7O)},    {"block8", whole(F_B8O)},
};

struct ConvSpec {
  std::string name;  // state_dict name without ".kernel"
  std::string bn;    // BN that follows ("" for final)
  int K, cin, cout;
  int64_t w_off = 0;   // offset of the kernel in the blob (floats)
  int64_t ss_off = 0;  // offset of scale/shift pair in the derived buffer
  int64_t wu_off = 0;  // offset of the unit-major permuted kernel (floats)
  int ds_cin = 0;      // > 0: this conv2 carries the block's fused 1x1 downsample (C_in of the block)
  int bn_idx = -1;     // its BN in NetSpec::bns (-1: final)
  int ds_idx = -1;     // ds_cin > 0: the block's 1x1 downsample conv in NetSpec::convs
  int nt() const { return (cout + 15) / 16; }
  int upk() const { return cin / 4; }
  int64_t wu_numel() const { return cin == 1 ? (int64_t)K * 16 : ((int64_t)K * upk() + ds_cin / 4) * nt() * 64; }
};
struct BnSpec {
  std::string name;
  int c;
  int64_t off = 0;  // weight, bias, running_mean, running_var consecutively
};
struct TensorInfo {
  std::string name;
  int64_t off, numel;
};

// One row per convolution of the forward pass, in forward order (minkunet.py:161-219): inference (forward_impl) and training
// (train_ops) both walk this table.  What is not in a row is derived from it:
//   * a block's conv2 names the block input `blk`: the residual where the block has no downsample (ds_cin == 0), else the
//     input of the 1x1 downsample -- fused into the conv2 launch at inference, a T_LIN op of its own before conv2 in training;
//   * the transposed convolution that SPS_FUSE_UP folds into a conv2's epilogue is the next row.
enum ConvKind { T_CONV0 = 0, T_K3 = 1, T_DOWN = 2, T_UP = 3, T_LIN = 4 };  // 5x5x5x1 on the constant input, 3x3x3x3, 2x2x2x1
                                                                            // stride 2, its transpose, 1x1 (training's downsample op)
struct LayerRow {
  ConvKind kind;
  int level;         // of the output rows (a stride-2 conv reads level - 1, a transposed one level + 1)
  FeatView in, out;  // out = relu?(bn(conv(in)) [+ block input])
  int relu;
  FeatView blk;      // conv2 of a block: the block's input
  int conv;          // index into NetSpec::convs
};

struct NetSpec {
  std::vector<ConvSpec> convs;
  std::vector<BnSpec> bns;
  std::vector<TensorInfo> tensors;
  std::vector<LayerRow> layers;
  std::string wiring_error;  // check_wiring: empty when the table is consistent
  int final_idx = -1;        // `final` in convs
  int64_t numel = 0, ss_numel = 0, bias_off = 0, wu_numel = 0;
  int out_channels = 1;  // C_out of `final` (1 = SPS / MapMOS, 3 = 4DMOS: c_ws/src/mos4d/scripts/mos4d.py:15)
};

int add_conv(NetSpec &s, const std::string &name, const std::string &bn, int K, int cin, int cout) {
  s.convs.push_back({name, bn, K, cin, cout});
  s.convs.back().bn_idx = (int)s.bns.size();
  s.bns.push_back({bn, cout});
  return (int)s.convs.size() - 1;
}

void add_block(NetSpec &s, const std::string &name, int cin, int cout, int level, FeatView in, FeatView mid, FeatView out) {
  const int c1 = add_conv(s, name + ".0.conv1", name + ".0.norm1", 81, cin, cout);
  const int c2 = add_conv(s, name + ".0.conv2", name + ".0.norm2", 81, cout, cout);
  if (cin != cout) {  // resnet.py:98
    const int ds = add_conv(s, name + ".0.downsample.0", name + ".0.downsample.1", 1, cin, cout);
    s.convs[c2].ds_cin = cin;
    s.convs[c2].ds_idx = ds;
  }
  s.layers.push_back({T_K3, level, in, mid, 1, FeatView{}, c1});
  s.layers.push_back({T_K3, level, mid, out, 1, in, c2});
}

// The table against the convolutions and the buffers it names; runs once per spec, on the host.  A message means a
// programming error in build_spec or FEAT: sps_ctx_create and sps_weights_create refuse to go on.
std::string check_wiring(const NetSpec &s) {
  auto fits = [](FeatView v) { return v.buf >= 0 && v.buf < N_FEAT && v.col0 >= 0 && v.cols > 0 && v.col0 + v.cols <= FEAT[v.buf].ld; };
  for (const LayerRow &r : s.layers) {
    if (r.conv < 0 || r.conv >= (int)s.convs.size()) return "a layer row names no convolution";
    const ConvSpec &cs = s.convs[r.conv];
    const int level_in = r.kind == T_DOWN ? r.level - 1 : r.kind == T_UP ? r.level + 1 : r.level;
    const int K = r.kind == T_CONV0 ? 125 : r.kind == T_K3 ? 81 : 8;
    const char *bad = nullptr;
    if (cs.bn_idx < 0 || cs.K != K || r.kind == T_LIN) bad = "is not the kind of convolution its row says";
    else if (!fits(r.out) || (r.kind != T_CONV0 && !fits(r.in))) bad = "has a view that does not fit its buffer";
    else if (cs.cin != r.in.cols) bad = "reads a view that is not C_in columns wide";
    else if (cs.cout != r.out.cols) bad = "writes a view that is not C_out columns wide";
    else if (r.level < 0 || r.level >= SPS_NUM_LEVELS || FEAT[r.out.buf].level != r.level) bad = "writes a buffer of another level";
    else if (r.kind != T_CONV0 && FEAT[r.in.buf].level != level_in) bad = "reads a buffer of another level";
    else if (cs.ds_cin > 0 && r.blk.buf < 0) bad = "needs the block input for its fused downsample";
    else if (r.blk.buf >= 0) {
      if (!fits(r.blk) || FEAT[r.blk.buf].level != r.level) bad = "has a block input that does not fit its buffer or level";
      else if (cs.ds_cin == 0 ? r.blk.cols != cs.cout
                              : (cs.ds_idx < 0 || s.convs[cs.ds_idx].cin != r.blk.cols || s.convs[cs.ds_idx].cout != cs.cout || cs.ds_cin != r.blk.cols))
        bad = "has a block input of the wrong width";
    }
    if (bad) return "layer table: " + cs.name + " " + bad;
  }
  if (s.final_idx < 0 || s.layers.empty() || s.convs[s.final_idx].cin != s.layers.back().out.cols) return "layer table: `final` does not follow the last layer";
  return "";
}

NetSpec build_spec(int out_channels) {
  NetSpec s;
  s.out_channels = out_channels;
  const int skip[4] = {PLANES[2], PLANES[1], PLANES[0], INIT_DIM};
  // the encoder output that decoder stage j concatenates sits behind the columns of that stage's transposed convolution
  auto skip_view = [&](int j) { return FeatView{F_CAT[j], PLANES[4 + j], skip[j]}; };
  FeatView x = skip_view(3);  // the running activation
  s.layers.push_back({T_CONV0, 0, FeatView{-1, 0, 1}, x, 1, FeatView{}, add_conv(s, "conv0p1s1", "bn0", 125, 1, INIT_DIM)});
  const char *downs[4] = {"conv1p1s2", "conv2p2s2", "conv3p4s2", "conv4p8s2"};
  int cur = INIT_DIM;
  for (int i = 0; i < 4; ++i) {
    const int level = i + 1;
    s.layers.push_back({T_DOWN, level, x, whole(F_X[i]), 1, FeatView{}, add_conv(s, downs[i], "bn" + std::to_string(i + 1), 8, cur, cur)});
    x = i < 3 ? skip_view(2 - i) : whole(F_BO[0]);
    add_block(s, "block" + std::to_string(i + 1), cur, PLANES[i], level, whole(F_X[i]), whole(F_BT[i]), x);
    cur = PLANES[i];
  }
  const char *ups[4] = {"convtr4p16s2", "convtr5p8s2", "convtr6p4s2", "convtr7p2s2"};
  for (int i = 0; i < 4; ++i) {
    const int level = 3 - i;
    s.layers.push_back({T_UP, level, x, FeatView{F_CAT[i], 0, PLANES[4 + i]}, 1, FeatView{},
                        add_conv(s, ups[i], "bntr" + std::to_string(4 + i), 8, cur, PLANES[4 + i])});
    x = whole(F_BO[1 + i]);
    add_block(s, "block" + std::to_string(5 + i), PLANES[4 + i] + skip[i], PLANES[4 + i], level, whole(F_CAT[i]), whole(F_BT[4 + i]), x);
    cur = PLANES[4 + i];
  }
  s.final_idx = (int)s.convs.size();
  s.convs.push_back({"final", "", 1, PLANES[7], out_channels});
  s.wiring_error = check_wiring(s);
  // blob layout: conv kernels, then BN (weight,bias,mean,var), then final.bias
  int64_t off = 0, ss = 0, wu = 0;
  for (auto &c : s.convs) {
    c.wu_off = wu;
    wu += c.wu_numel();
    c.w_off = off;
    const int64_t n = (int64_t)c.K * c.cin * c.cout;
    s.tensors.push_back({c.name + ".kernel", off, n});
    off += n;
    c.ss_off = ss;
    ss += 2 * c.cout;
  }
  const char *bn_parts[4] = {".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var"};
  for (auto &b : s.bns) {
    b.off = off;
    for (int j = 0; j < 4; ++j) {
      s.tensors.push_back({b.name + bn_parts[j], off, b.c});
      off += b.c;
    }
  }
  s.bias_off = off;
  s.tensors.push_back({"final.bias", off, out_channels});
  off += out_channels;
  s.numel = off;
  s.ss_numel = ss;
  s.wu_numel = wu;
  return s;
}

constexpr int MAX_HEAD = 8;  // `final` C_out supported by the head path (one 8-wide row of block8's output)

// spec(1) is the SPS network; spec(k) differs only in final.kernel [8,k] / final.bias [k] (and the offsets after them)
const NetSpec &spec(int out_channels = 1) {
  static const std::vector<NetSpec> all = [] {
    std::vector<NetSpec> v;
    for (int k = 1; k <= MAX_HEAD; ++k) v.push_back(build_spec(k));
    return v;
  }();
  return all[(size_t)(out_channels < 1 ? 1 : (out_channels > MAX_HEAD ? MAX_HEAD : out_channels)) - 1];
}

