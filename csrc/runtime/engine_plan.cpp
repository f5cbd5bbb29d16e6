// The engine's launch planner (see engine.h): which kernel runs which ops of
// one forward (Engine::plan), the conv geometry its predicates read, and the
// plan as text (plan_audit, plan_lines).
#include "engine.h"

#include <algorithm>
#include <stdexcept>

namespace dmlc {

namespace {
// conv1x1.hip's *_supported checks read res, x2 and the chained reduce's
// alpha / bias / w / y only as "the launch has this operand". A geometry has
// no operands yet, so conv_geom marks the ones the layer has with this; bind()
// replaces every one of them.
alignas(16) char g_operand[16];
}  // namespace

ConvArgs Engine::conv_geom(const Op& op, int B) const {
  const ConvLayer& L = convs_[op.conv];
  const ActShape& is = shapes_[op.in];
  const ActShape& os = shapes_[op.out];
  ConvArgs a;
  a.w = a.y = g_operand;
  a.bias = (const float*)g_operand;
  if (op.res >= 0) a.res = g_operand;
  if (L.fp8) a.alpha = (const float*)g_operand;
  a.stem = L.pair;
  a.B = B;
  if (L.fc) {
    a.H = a.W = 1;
    a.Cin = L.cin_eff;
  } else {
    a.H = is.H;
    a.W = is.W;
    a.Cin = is.C;
  }
  a.KH = L.kh;
  a.KW = L.kw;
  a.stride = L.stride;
  a.pad = L.pad;
  a.Ho = os.H;
  a.Wo = os.W;
  a.N = L.cout;
  a.Npad = L.npad;
  a.Kpad = L.kpad;
  a.ldo = L.cout;
  a.relu = L.relu;
  a.out_f32 = os.f32;
  a.in_fp8 = L.fp8;
  a.out_fp8 = os.fp8;
  if (op.res >= 0 && shapes_[op.res].fp8) a.res_scale = shapes_[op.res].scale;
  if (os.fp8) a.out_inv_scale = 1.f / os.scale;
  int s = conv_pick_split_k(a, num_cus_);
  const size_t M = (size_t)B * os.H * os.W;
  if (opt_.igemm_small_m && M <= 1024 && !L.pair && !L.fc && !L.fp8 && !os.fp8 && !os.f32 && L.npad % 128 == 0) {
    // 64x256 ns3 for the narrowest outputs, else 128x128 ns3 (conv_igemm.hip tile table)
    a.tile = (M <= 64 && L.npad % 256 == 0) ? 5 : 3;
    const int bm = a.tile == 5 ? 64 : 128, bn = a.tile == 5 ? 256 : 128;
    const int tiles = (int)((M + bm - 1) / bm) * (L.npad / bn);
    const int k_tiles = L.kpad / 64;
    s = std::max(1, std::min({k_tiles / 2, (num_cus_ / 2 + tiles - 1) / tiles, 32}));
  }
  while (s > 1 && (size_t)s * M * L.npad > kSplitKWsElems) --s;
  a.split_k = s;
  a.persistent = opt_.persistent;
  a.max_blocks = 2 * num_cus_;
  return a;
}

// A resnet50_fp8 layer1 identity bottleneck's expand conv (1x1, 64 -> 256 on
// 56x56, bf16 in, e4m3 out): bottleneck56.hip reads its weights in fragment order.
bool Engine::bottleneck_conv3(const ConvLayer& L) const {
  if (!L.plain() || L.kh != 1 || L.kw != 1 || L.stride != 1) return false;
  const ActShape& is = shapes_[L.in_act];
  return fp8_ && is.C == 64 && L.cout == 256 && L.kpad == 64 && bottleneck56_supported(is.H, is.W, 256, 64);
}

const char* kernel_name(Kernel k) {
  static const char* const names[] = {
      "None", "AlexStem", "StemPoolU8", "StemPool", "FcSmall", "Conv1x1Cat", "Conv1x1Chain", "Bottleneck56",
      "Bottleneck56Head", "Block", "S2Rows", "S2Rows128", "Stream", "Stream8", "Rows28", "Rows", "Small", "Direct13",
      "Direct27", "Conv1x1", "BigTile", "Igemm", "FcGemm", "HeadPooled", "HeadFused", "AvgPoolGlobal",
      "AvgPoolAdaptive", "MaxPool", "Preprocess", "PackTensor", "SoftmaxTop1", "SoftmaxTopK", "Embed"};
  static_assert(sizeof(names) / sizeof(names[0]) == (size_t)Kernel::Embed + 1, "one name per Kernel");
  return names[(size_t)k];
}

// ---------------------------------------------------------------- planner
// What to launch for one forward of B images: each conv op's kernel path
// (once per plan), then one walk over the ops that decides which neighbours a
// launch swallows. Reads the graph, the layout pass's results (frag, cat_off,
// npad) and num_cus_; no device state.
struct Engine::Planner {
  enum class Path { Stream, Rows, Rows28, Direct13, Direct27, OneByOne, BigTile, Igemm, Small, Stream8, Fc };

  const Engine& e;
  const std::vector<Op>& ops;
  const std::vector<ConvLayer>& convs;
  const std::vector<ActShape>& shapes;
  const EngineOptions& opt;
  const int B, cus;
  std::vector<Path> path;    // per conv op
  std::vector<int> cat_ds;   // per op: the downsample op this expand conv computes itself (conv1x1 x2), or -1
  std::vector<int> cat_by;   // per op: the expand conv that computes this downsample, or -1
  std::vector<Step> steps;
  int skip_ds = -1;     // downsample op left to the next op (the block's stride-2 conv1)
  int ds_conv2 = -1;    // downsample op left to the block's conv2 (ds_into_conv2)
  bool pooled = false;  // the last conv's epilogue wrote the global average pool

  Planner(const Engine& eng, int batch)
      : e(eng), ops(eng.ops_), convs(eng.convs_), shapes(eng.shapes_), opt(eng.opt_), B(batch), cus(eng.num_cus_),
        path(ops.size(), Path::Igemm), cat_ds(ops.size(), -1), cat_by(ops.size(), -1) {
    for (size_t i = 0; i < ops.size(); ++i) {
      if (ops[i].type != OpType::Conv) continue;
      path[i] = conv_path(ops[i]);
      const int r = ds_expand_op(i);
      cat_by[i] = r;
      if (r > (int)i) cat_ds[r] = (int)i;
    }
  }

  bool conv(size_t i) const { return i < ops.size() && ops[i].type == OpType::Conv; }
  // the only reader of activation a is op j
  bool only_reader(int a, size_t j) const {
    for (size_t i = 0; i < ops.size(); ++i)
      if (i != j && (ops[i].in == a || ops[i].res == a)) return false;
    return true;
  }
  // one-workgroup-per-image kernels: only with rounds of num_cus images that are >= ~70% full
  bool full_rounds() const { return 10 * B >= 7 * ((B + cus - 1) / cus) * cus; }

  Path conv_path(const Op& op) const {
    const ConvLayer& L = convs[op.conv];
    const ActShape& is = shapes[op.in];
    const bool k3b = L.plain_3x3() && !shapes[op.out].f32;
    const bool k3 = k3b && !shapes[op.out].fp8;
    // e4m3 output (fp8_3x3_out): the row / stream kernels' e4m3 epilogue
    const bool k3o8 = k3b && shapes[op.out].fp8 && opt.fp8_3x3_out && op.res < 0;
    // the stream conv runs 1-4 workgroups per image (or image pair): only
    // worth it once the batch fills the CUs
    // 14x14x256 -> 7x7x512 / s2 (layer4.0.conv1) runs 2 rounds of single-image
    // workgroups with 49 of 64 fragment rows live: with the LDS weight ring and
    // the fused downsample 67.9 us vs 44.2 + 13.3 us as two implicit GEMMs; with
    // register weights 48.1 vs 13.2 + 46.3 us (profiles/r1_fused_ds.txt)
    const bool l4s2 = L.stride == 2 && is.H < 28 && !(opt.stream_l4s2 && opt.stream_wreg);
    const bool l1 = L.stride == 1 && is.C == 64;  // layer1: conv3x3_rows (the stream conv measured slower there)
    // query batches: one launch per conv, no split-K (conv_small.hip)
    if (opt.small_conv && k3 && L.frag == FragOrder::Stream && B <= kSmallConvMaxB &&
        conv_small_supported(is.H, is.W, is.C, L.cout, L.stride) &&
        !(opt.direct13 && conv3x3_13_supported(is.H, is.W, is.C, L.cout)))  // (AlexNet keeps its fused pools)
      return Path::Small;
    // layer2's stride-1 convs: one weight-stationary workgroup per image walking
    // its rows (59-60 us vs 62-66 us for the stream conv at B=256,
    // profiles/r2_rows28.txt)
    if (opt.rows28 && (k3 || k3o8) && L.stride == 1 && L.frag == FragOrder::Stream && full_rounds() &&
        conv3x3_rows28_supported(is.H, is.W, is.C, L.cout))
      return Path::Rows28;
    if (opt.direct13 && k3 && L.stride == 1 && L.frag == FragOrder::Stream &&
        conv3x3_13_supported(is.H, is.W, is.C, L.cout))
      return Path::Direct13;
    // e4m3 in and out (fp8_3x3_in): whole images per workgroup, once the batch
    // fills the CUs (query batches: the e4m3 implicit GEMM)
    if (L.fp8 && !L.fc && L.kh == 3 && L.kw == 3 && L.pad == 1 && L.frag == FragOrder::Stream8 && op.res < 0 &&
        shapes[op.out].fp8 && 4 * B >= cus && conv3x3_stream8_supported(is.H, is.W, is.C, L.cout, L.stride))
      return Path::Stream8;
    if (opt.direct27 && L.plain() && L.kh == 5 && L.kw == 5 && L.stride == 1 && L.relu && L.frag == FragOrder::Stream &&
        L.kpad == 1600 && !shapes[op.out].f32 && conv5x5_27_supported(is.H, is.W, is.C, L.cout, L.pad))
      return Path::Direct27;
    if (opt.stream_conv && (k3 || k3o8) && !l4s2 && !l1 && 8 * B >= cus &&
        conv3x3_stream_supported(is.H, is.W, is.C, L.cout, L.stride))
      return Path::Stream;
    if (opt.row_conv && k3 && L.stride == 1 && conv3x3_rows_supported(is.H, is.W, is.C, L.cout)) return Path::Rows;
    if (opt.conv1x1 && !L.fc && L.kh == 1 && L.kw == 1) {
      ConvArgs a = e.conv_geom(op, B);
      a.split_k = 1;
      if (conv1x1_supported(a)) return Path::OneByOne;
    }
    if (opt.fc_gemm && L.fc && !L.fp8 && fc_gemm_supported(e.conv_geom(op, B)) &&
        (size_t)B * L.npad <= kSplitKWsElems)
      return Path::Fc;
    if (opt.bigtile && conv_bigtile_pick(e.conv_geom(op, B), cus) >= 0) return Path::BigTile;
    return Path::Igemm;
  }

  // ops[oi] is a downsample whose only reader is a later expand conv that
  // computes it itself (its cat_ds, the K-concat form of conv1x1): that op's
  // index, else -1.
  int ds_expand_op(size_t oi) const {
    if (!opt.ds_into_expand) return -1;
    const Op& d = ops[oi];
    int reader = -1;
    for (size_t j = 0; j < ops.size() && reader < 0; ++j)
      if (j != oi && ops[j].res == d.out) reader = (int)j;
    if (reader < 0 || ops[reader].in == d.out || !only_reader(d.out, reader)) return -1;
    const ConvLayer& L3 = convs[ops[reader].conv];
    if (L3.cat_ds != d.conv || !L3.cat_off) return -1;
    const ConvLayer& D = convs[d.conv];
    ConvArgs a = e.conv_geom(ops[reader], 1);
    a.split_k = 1;
    a.res = nullptr;
    a.x2 = g_operand;
    a.cin2 = D.cin;
    a.Kpad = L3.kpad + D.kpad;
    return conv1x1_supported(a) ? reader : -1;
  }

  bool head_fusable(size_t oi) const {
    if (!opt.fused_head || oi + 2 >= ops.size()) return false;
    const Op& pool = ops[oi];
    const Op& fc = ops[oi + 1];
    const Op& sm = ops[oi + 2];
    if (pool.type != OpType::AvgPoolGlobal || fc.type != OpType::Conv || sm.type != OpType::SoftmaxTop1) return false;
    if (fc.in != pool.out || sm.in != fc.out || !shapes[fc.out].f32 || shapes[pool.out].fp8) return false;
    const ConvLayer& L = convs[fc.conv];
    // (an e4m3 pool input, ResNet50 fp8: pooled from e4m3 in the head, C >= 2048)
    if (shapes[pool.in].fp8 && shapes[pool.in].C < 2048) return false;
    return L.fc && !L.fp8 && !L.relu && L.cin == shapes[pool.in].C && head_supported(L.cin, L.cout, L.kpad, L.npad);
  }

  // ops[oi] is the last conv (stream path, whole-image workgroups) and
  // ops[oi+1] the global average pool, the only reader of its output: the
  // conv's epilogue writes the pooled bf16 vectors straight into the pool's
  // output activation (and, under a graph, skips storing its own).
  bool pool_fusable(size_t oi) const {
    if (!opt.fused_pool || oi + 1 >= ops.size()) return false;
    const Op& c = ops[oi];
    const Op& p = ops[oi + 1];
    if (p.type != OpType::AvgPoolGlobal || p.in != c.out) return false;
    if (shapes[p.out].fp8 || shapes[p.out].f32 || shapes[p.in].fp8 || !only_reader(c.out, oi + 1)) return false;
    const ConvLayer& L = convs[c.conv];
    const ActShape& is = shapes[c.in];
    return !L.fp8 && path[oi] == Path::Stream && conv3x3_stream_pool_supported(is.H, is.W, is.C, L.cout, L.stride);
  }

  // ops[oi] is a block's downsample (1x1/s2, BN, no ReLU) and ops[oi+1] the
  // block's 3x3/s2 conv1 on the same input, run by the stream conv (or the
  // query-batch conv, which needs the downsample's fragment-order weights).
  bool ds_fusable(size_t oi) const {
    if (!conv(oi + 1)) return false;
    const Op& d = ops[oi];
    const Op& c = ops[oi + 1];
    const ConvLayer& D = convs[d.conv];
    const ConvLayer& L = convs[c.conv];
    return d.in == c.in && D.plain_ds2() && !D.relu && d.res < 0 && D.cout == L.cout && L.stride == 2 &&
           !shapes[d.out].fp8 && !shapes[d.out].f32 &&
           (path[oi + 1] == Path::Stream || (path[oi + 1] == Path::Small && D.frag == FragOrder::Stream));
  }

  // ops[oi], ops[oi+1] = conv1 (+ReLU) and conv2 (+identity residual, ReLU) of
  // a 56x56x64 basic block, both on the register-weight row conv, and conv1's
  // output read by nothing else: conv3x3_block runs the pair with the
  // intermediate kept in LDS (not written to its activation).
  // One workgroup per image walks all 56 rows (~100 us per round of num_cus
  // images at B=256 vs ~2 x 72 us for the two row convs, which split images
  // into strips; B=1: 86 us fused vs ~30 us as strips;
  // profiles/r2_block_kernel_stats.txt).
  bool block_fusable(size_t oi) const {
    if (!opt.fused_block || !opt.rows_wreg || !full_rounds() || !conv(oi + 1)) return false;
    const Op& c1 = ops[oi];
    const Op& c2 = ops[oi + 1];
    if (c2.in != c1.out || c1.res >= 0 || c2.res != c1.in || c1.side || c2.side || !only_reader(c1.out, oi + 1))
      return false;
    const ConvLayer& L1 = convs[c1.conv];
    const ConvLayer& L2 = convs[c2.conv];
    const ActShape& is = shapes[c1.in];
    return L1.relu && L2.relu && L1.frag == FragOrder::Stream && L2.frag == FragOrder::Stream &&
           conv3x3_block_supported(is.H, is.W, is.C) && L1.cout == is.C && L2.cout == is.C && !shapes[c1.in].fp8 &&
           !shapes[c2.out].fp8 && path[oi] == Path::Rows && path[oi + 1] == Path::Rows;
  }

  // a layer1 bottleneck's 3x3 (64 -> 64 on 56x56, fragment-order weights), as bottleneck56.hip runs it
  static bool bottleneck_conv2(const ConvLayer& L2) {
    return L2.kh == 3 && L2.kw == 3 && L2.stride == 1 && L2.pad == 1 && L2.relu && L2.cout == 64 &&
           L2.frag == FragOrder::Stream && L2.kpad == 576;
  }

  // ops[oi..oi+2] = conv1 (1x1 256 -> 64, e4m3 in) + conv2 (3x3 64 -> 64) +
  // conv3 (1x1 64 -> 256 + the block input as residual, e4m3 out) of a
  // resnet50_fp8 layer1 identity block, the intermediates read by nothing else.
  bool bottleneck_fusable(size_t oi) const {
    if (!opt.fused_bottleneck || !e.fp8_ || !conv(oi + 1) || !conv(oi + 2)) return false;
    const Op& c1 = ops[oi];
    const Op& c2 = ops[oi + 1];
    const Op& c3 = ops[oi + 2];
    if (c1.side || c2.side || c3.side || c2.in != c1.out || c3.in != c2.out || c1.res >= 0 || c2.res >= 0 ||
        c3.res != c1.in)
      return false;
    const ConvLayer& L1 = convs[c1.conv];
    const ConvLayer& L3 = convs[c3.conv];
    const ActShape& xs = shapes[c1.in];
    if (!xs.fp8 || !shapes[c3.out].fp8 || shapes[c1.out].fp8 || shapes[c2.out].fp8) return false;
    if (!bottleneck56_supported(xs.H, xs.W, xs.C, L1.cout) || !L1.fp8 || L1.kh != 1 || L1.stride != 1 || !L1.relu ||
        L1.kpad != 256 || L1.npad != 64)
      return false;
    if (!bottleneck_conv2(convs[c2.conv]) || !e.bottleneck_conv3(L3) || L3.frag != FragOrder::Stream || !L3.relu)
      return false;
    return only_reader(c1.out, oi + 1) && only_reader(c2.out, oi + 2);
  }

  // ops[oi], ops[oi+1] = layer1.0's reduce 1x1 (64 -> 64) + 3x3 -> bottleneck56_head
  bool bottleneck_head_fusable(size_t oi) const {
    if (!opt.fused_bottleneck || !conv(oi + 1)) return false;
    const Op& c1 = ops[oi];
    const Op& c2 = ops[oi + 1];
    if (c1.side || c2.side || c2.in != c1.out || c1.res >= 0 || c2.res >= 0) return false;
    const ConvLayer& L1 = convs[c1.conv];
    const ConvLayer& L2 = convs[c2.conv];
    const ActShape& xs = shapes[c1.in];
    if (xs.fp8 || xs.f32 || shapes[c1.out].fp8 || shapes[c2.out].fp8 || shapes[c2.out].f32) return false;
    if (!bottleneck56_supported(xs.H, xs.W, 256, 64) || xs.C != 64) return false;
    if (L1.fc || L1.fp8 || L1.pair || L1.stem_pool || L1.kh != 1 || L1.kw != 1 || L1.stride != 1 || !L1.relu ||
        L1.cout != 64 || L1.kpad != 64 || L1.npad != 64)
      return false;
    return !L2.fp8 && bottleneck_conv2(L2) && only_reader(c1.out, oi + 1);
  }

  // ops[oi] (with its downsample D left to it: fuse_ds) is layer2.0's conv1 on
  // the 56x56x64 -> 128 shape: conv3x3_s2rows runs one workgroup per image
  // (59 us at B=256 vs 72 us for the stream conv's 4 rounds of strips,
  // profiles/r2_s2rows.txt).
  bool s2rows_ok(const Op& op, const ConvLayer& D) const {
    const ConvLayer& L = convs[op.conv];
    const ActShape& is = shapes[op.in];
    return opt.s2rows && op.res < 0 && L.frag == FragOrder::Stream && D.frag == FragOrder::Stream && full_rounds() &&
           conv3x3_s2rows_supported(is.H, is.W, is.C, L.cout);
  }

  // ... and ops[oi - 1] its downsample: the block's conv2 (ops[oi + 1], on
  // conv3x3_rows28) can compute that downsample as 2 more K steps when it is
  // the downsample output's only reader (ds_into_conv2).
  bool ds_conv2_ok(size_t oi) const {
    if (!opt.ds_into_conv2 || oi < 1 || !conv(oi + 1)) return false;
    const Op& d = ops[oi - 1];
    const Op& c2 = ops[oi + 1];
    if (c2.res != d.out || c2.in != ops[oi].out) return false;
    const ConvLayer& L2 = convs[c2.conv];
    const ConvLayer& D = convs[d.conv];
    if (L2.frag != FragOrder::Stream || D.frag != FragOrder::Stream || L2.fp8 || shapes[c2.out].fp8 ||
        path[oi + 1] != Path::Rows28)
      return false;
    const ActShape& xs = shapes[d.in];
    if (xs.H != 56 || xs.W != 56 || xs.C != 64 || xs.fp8 || xs.f32 || L2.cout != 128 || D.cout != 128) return false;
    return only_reader(d.out, oi + 1);
  }

  // ops[oi] is a bottleneck's expand conv (1x1, residual) and ops[oi + 1] the
  // next bottleneck's reduce conv on its output, both on conv1x1.hip, in a form
  // conv1x1_chain runs as one launch (ResNet50 e4m3 layer2.0-2.2 -> 2.1-2.3).
  // The expand output keeps its other reader (the next expand's residual).
  bool chain_ok(size_t oi) const {
    if (!opt.chain_1x1 || !conv(oi + 1)) return false;
    const Op& x = ops[oi];
    const Op& r = ops[oi + 1];
    if (x.res < 0 || r.in != x.out || r.res >= 0 || x.side || r.side) return false;
    if (path[oi] != Path::OneByOne || path[oi + 1] != Path::OneByOne) return false;
    if (convs[x.conv].cat_off) return false;  // (an expand with its downsample as a second K block)
    ConvArgs a = e.conv_geom(x, B), ra = e.conv_geom(r, B);
    a.split_k = ra.split_k = 1;
    return conv1x1_chain_supported(a, ra);
  }

  // AlexNet: the 3x3/s2 max-pool ops[oi + 1] (to out x out) in conv ops[oi]'s
  // epilogue, when the pool is the conv output's only reader
  bool maxpool_fusable(size_t oi, int out) const {
    if (!opt.fused_pool || oi + 1 >= ops.size()) return false;
    const Op& mp = ops[oi + 1];
    return mp.type == OpType::MaxPool && mp.in == ops[oi].out && mp.k == 3 && mp.stride == 2 && mp.pad == 0 &&
           shapes[mp.out].H == out && shapes[mp.out].W == out && only_reader(ops[oi].out, oi + 1);
  }

  Step& emit(Kernel k, size_t first, int n) {
    Step st;
    st.kernel = k;
    st.first_op = (int)first;
    st.n_ops = n;
    steps.push_back(st);
    return steps.back();
  }

  void plan_conv(size_t oi, bool side_ready, bool keep_acts) {
    const Op& op = ops[oi];
    const ConvLayer& L = convs[op.conv];
    const ActShape& is = shapes[op.in];
    if (cat_by[oi] >= 0) {  // computed by its expand conv (conv1x1 x2)
      emit(Kernel::None, oi, 1);
      return;
    }
    if (opt.fuse_ds && op.side && ds_fusable(oi)) {  // computed by the next op (the block's stride-2 conv1)
      skip_ds = (int)oi;
      emit(Kernel::None, oi, 1);
      return;
    }
    // A downsample conv may run on the side stream, concurrently with its
    // block's conv1 (both read the block input; conv2 joins them through the
    // residual). The fused multi-op kernels stay on the main stream.
    const bool side = side_ready && op.side;
    // query-sized batches: weight-streaming GEMV (AlexNet classifier)
    if (L.fc && !L.fp8 && !shapes[op.out].fp8 && opt.fc_small && fc_small_supported(B, L.cin, L.cin, L.kpad)) {
      emit(Kernel::FcSmall, oi, 1).side = side;
      return;
    }
    if (L.cat_off && op.res >= 0 && cat_ds[oi] >= 0) {  // expand conv + its stride-1 downsample as one K-concatenated GEMM
      Step& st = emit(Kernel::Conv1x1Cat, oi, 1);
      st.ds_op = cat_ds[oi];
      st.side = side;
      return;
    }
    if (!side) {
      if (chain_ok(oi)) return (void)emit(Kernel::Conv1x1Chain, oi, 2);
      if (bottleneck_fusable(oi)) return (void)emit(Kernel::Bottleneck56, oi, 3);
      if (bottleneck_head_fusable(oi)) return (void)emit(Kernel::Bottleneck56Head, oi, 2);
      if (block_fusable(oi)) return (void)emit(Kernel::Block, oi, 2);
    }
    Step& st = emit(Kernel::Igemm, oi, 1);
    st.side = side;
    const int ds = (skip_ds >= 0 && skip_ds + 1 == (int)oi) ? skip_ds : -1;  // its block's downsample, left to it
    const ConvLayer* D = ds >= 0 ? &convs[ops[ds].conv] : nullptr;
    switch (path[oi]) {
      case Path::Stream: {
        if (D && s2rows_ok(op, *D)) {
          st.kernel = Kernel::S2Rows;
          if (ds_conv2_ok(oi))
            ds_conv2 = ds;  // the downsample runs inside conv2
          else
            st.ds_op = ds;
          break;
        }
        // ResNet50 layer2.0.conv2: one weight-stationary workgroup per image
        if (!D && opt.s2rows128 && op.res < 0 && L.frag == FragOrder::Stream && L.stride == 2 && full_rounds() &&
            conv3x3_s2rows128_supported(is.H, is.W, is.C, L.cout)) {
          st.kernel = Kernel::S2Rows128;
          break;
        }
        st.kernel = Kernel::Stream;
        st.ds_op = ds;
        // (the copy may exist for conv3x3_s2rows alone)
        st.wreg = L.frag == FragOrder::Stream && opt.stream_wreg && (!D || D->frag == FragOrder::Stream) &&
                  conv3x3_stream_uses_frag(is.H, is.W, is.C, L.cout, L.stride);
        pooled = !side && pool_fusable(oi);
        if (pooled) {
          st.pool_op = (int)oi + 1;
          st.store_y = keep_acts;  // eager / profile runs keep the activation (tests read it)
        }
        break;
      }
      case Path::Direct13:  // AlexNet features.10 + features.12
        st.kernel = Kernel::Direct13;
        if (!side && L.relu && conv3x3_13_pool_supported(is.C, L.cout) && maxpool_fusable(oi, 6)) {
          st.pool_op = (int)oi + 1;
          st.n_ops = 2;
        }
        break;
      case Path::Direct27:  // AlexNet features.3 + features.5
        st.kernel = Kernel::Direct27;
        if (!side && maxpool_fusable(oi, 13)) {
          st.pool_op = (int)oi + 1;
          st.n_ops = 2;
        }
        break;
      case Path::Small:
        st.kernel = Kernel::Small;
        st.ds_op = ds;
        st.count = conv_small_pick_mf(B, is.H, is.W, is.C, L.cout, L.stride, cus);
        break;
      case Path::Stream8:
        st.kernel = Kernel::Stream8;
        break;
      case Path::Rows28:
        st.kernel = Kernel::Rows28;
        if (ds_conv2 >= 0 && op.res == ops[ds_conv2].out) {
          st.ds_op = ds_conv2;
          ds_conv2 = -1;
        }
        break;
      case Path::Rows:
        st.kernel = Kernel::Rows;
        st.wreg = L.frag == FragOrder::Stream && opt.rows_wreg;
        st.count = conv3x3_rows_pick_strip(B, is.H, st.wreg ? 2 * cus : cus);
        break;
      case Path::OneByOne:
        st.kernel = Kernel::Conv1x1;
        break;
      case Path::BigTile: {
        const ConvArgs a = e.conv_geom(op, B);
        st.kernel = Kernel::BigTile;
        st.cfg = conv_bigtile_pick(a, cus);
        st.count = conv_bigtile_splits(a, st.cfg, cus);  // (run_ops: 1 if the reserved slab is too small)
        break;
      }
      case Path::Igemm:
        break;
      case Path::Fc: {
        if (side) break;  // (its partials need the main stream's split-K workspace): the implicit GEMM
        const ConvArgs a = e.conv_geom(op, B);
        st.kernel = Kernel::FcGemm;
        st.count = fc_gemm_splits(a, cus);
        while (st.count > 1 && ((size_t)st.count * B * a.Npad > kSplitKWsElems || (a.Kpad / 64) % st.count))
          --st.count;
        break;
      }
    }
  }

  // the step that does op oi (a launch, or None for an op another step computes)
  const Step& step_of(int oi) const {
    for (const Step& st : steps)
      if (st.n_ops > 0 && st.first_op <= oi && oi < st.first_op + st.n_ops) return st;
    throw std::logic_error("plan: no step for op " + ops[oi].name);
  }
  // Op oi's output activation is known to be in memory after the plan's
  // steps: a conv's epilogue pooled into it, or it is the last op of a launch
  // that stores its output (an inner op's may stay on chip: HeadFused's pooled
  // vector, a fused block's intermediate).
  bool stored(int oi) const {
    for (const Step& st : steps)
      if (st.pool_op == oi) return true;
    const Step& st = step_of(oi);
    return st.kernel != Kernel::None && oi == st.first_op + st.n_ops - 1 && st.store_y;
  }

  // The Embed step (header: Engine::plan). F = the input of the fc that
  // writes the logits.
  void plan_embed() {
    int fc = -1;
    for (size_t i = 0; i < ops.size(); ++i)
      if (ops[i].type == OpType::Conv && ops[i].out == e.logits_act_) fc = (int)i;
    if (fc < 0) throw std::logic_error("features: no fc writes the logits");
    int prod = -1;  // the op that writes F
    for (size_t i = 0; i < ops.size(); ++i)
      if (ops[i].out == ops[fc].in) prod = (int)i;
    if (prod < 0) throw std::logic_error("features: nothing writes the fc's input");
    Step st;
    st.kernel = Kernel::Embed;
    st.first_op = (int)ops.size() - 1;
    st.n_ops = 0;
    const ActShape& fs = shapes[ops[prod].out];
    if (stored(prod)) {
      if (fs.f32 || fs.fp8 || !embed_rows_supported(1, (int)fs.elems_per_image()))
        throw std::logic_error("features: the fc's input is no bf16 row embed_rows reads");
      st.src_op = prod;
    } else {
      // only HeadFused leaves F unwritten; it pools ops[prod].in, which a step
      // stores (store_y is false only where the pool is fused, and then F exists)
      const Op& pool = ops[prod];
      if (step_of(prod).kernel != Kernel::HeadFused || pool.type != OpType::AvgPoolGlobal)
        throw std::logic_error("features: the fc's input is not stored and no fused head pools it");
      int src = -1;
      for (size_t i = 0; i < ops.size(); ++i)
        if (ops[i].out == pool.in) src = (int)i;
      const ActShape& is = shapes[pool.in];
      if (src < 0 || !stored(src)) throw std::logic_error("features: the fused head's input is not stored");
      if (is.f32 || !is.cscale.empty() || is.H * is.W < 2 || !embed_rows_supported(is.H * is.W, is.C))
        throw std::logic_error("features: embed_rows cannot pool the fused head's input");
      st.src_op = src;
      st.count = is.H * is.W;
    }
    steps.push_back(st);
  }

  std::vector<Step> run(const PlanSpec& spec) {
    // a float tensor takes the resized-input plan: the u8 stems cannot read it
    const bool tensor_in = spec.tensor_in, native = spec.native && !tensor_in;
    // never a side stream next to a big-tile conv
    const bool side_ready = spec.side && std::find(path.begin(), path.end(), Path::BigTile) == path.end();
    for (size_t oi = 0; oi < ops.size(); oi = steps.back().first_op + steps.back().n_ops) {
      const Op& op = ops[oi];
      switch (op.type) {
        case OpType::Preprocess:
          // AlexNet: 224x224 u8 images -> features.2's output in one kernel
          if (native && opt.fused_preprocess && conv(oi + 1) && oi + 2 < ops.size() &&
              ops[oi + 2].type == OpType::MaxPool && convs[ops[oi + 1].conv].alex_stem)
            emit(Kernel::AlexStem, oi, 3);
          // images already SxS feed the fused stem directly (StemPoolU8)
          else if (native && opt.fused_preprocess && op.k == 1)
            emit(Kernel::None, oi, 1);
          else
            emit(tensor_in ? Kernel::PackTensor : Kernel::Preprocess, oi, 1);
          break;
        case OpType::Conv:
          plan_conv(oi, side_ready, spec.keep_acts);
          break;
        case OpType::StemPool: {
          const ConvLayer& L = convs[op.conv];
          const int PH = shapes[op.out].H;
          if (native && opt.fused_preprocess) {
            Step& st = emit(Kernel::StemPoolU8, oi, 1);
            st.count = opt.stem_roles ? stem_pool_u8_pick_strip(B, PH, cus) : stem_pool_pick_strip(B, PH, cus);
            st.wreg = opt.stem_dense && L.frag == FragOrder::StemDense;
          } else {
            emit(Kernel::StemPool, oi, 1).count = stem_pool_pick_strip(B, PH, cus);
          }
          break;
        }
        case OpType::MaxPool:
          emit(Kernel::MaxPool, oi, 1);
          break;
        case OpType::AvgPoolGlobal:
          if (pooled) {  // pooled by the last conv's epilogue; fc + softmax / top-1 in one launch, or as ops
            emit(Kernel::None, oi, 1);
            if (head_fusable(oi)) emit(Kernel::HeadPooled, oi + 1, 2);
          } else if (head_fusable(oi) && B >= kPoolThenHeadB) {
            // throughput batches: pool once, then fc + softmax/top-1 on the
            // pooled rows (head_fused pools its images again in every class
            // split: resnet50_fp8 b256 86 us, 8 x 25.7 MB of e4m3 reads)
            emit(Kernel::AvgPoolGlobal, oi, 1);
            emit(Kernel::HeadPooled, oi + 1, 2);
          } else if (head_fusable(oi)) {  // avgpool + fc + softmax/top-1 in one launch
            emit(Kernel::HeadFused, oi, 3);
          } else {
            emit(Kernel::AvgPoolGlobal, oi, 1);
          }
          break;
        case OpType::AvgPoolAdaptive:
          emit(Kernel::AvgPoolAdaptive, oi, 1);
          break;
        case OpType::SoftmaxTop1:
          emit(Kernel::SoftmaxTop1, oi, 1);
          break;
      }
    }
    // top-k: the plan above unchanged (its tail still writes the logits and a
    // top-1 of its own), then the ranking of those logits
    if (spec.topk > 1) emit(Kernel::SoftmaxTopK, ops.size() - 1, 0).count = spec.topk;
    // features: the plan above unchanged, then the fc's input as fp32 rows
    if (spec.features) plan_embed();
    return std::move(steps);
  }
};

void Engine::check_topk(int k) const {
  if (k < 1 || k > std::min(num_classes_, kMaxTopK))
    throw std::invalid_argument("top-k: k must be in 1..min(num_classes, " + std::to_string(kMaxTopK) + ")");
}

std::vector<Step> Engine::plan(const PlanSpec& spec) const {
  check_topk(spec.topk);
  return Planner(*this, spec.B).run(spec);
}

PlanSpec Engine::spec_for(const Request& req, bool keep_acts) const {
  PlanSpec spec;
  spec.B = req.B;
  spec.native = req.in.Hin == image_size_ && req.in.Win == image_size_;
  spec.side = opt_.fork_ds;
  spec.keep_acts = keep_acts;
  spec.topk = req.k;
  spec.tensor_in = req.in.tensor;
  spec.features = req.features != nullptr;
  return spec;
}

Engine::GraphKey Engine::key_of(const Request& req) {
  return GraphKey{req.in.data, req.B, req.in.Hin, req.in.Win, req.idx, req.prob, req.logits, req.k, req.in.kind(),
                  req.features, req.features && req.l2norm};
}

std::string Engine::step_detail(const Step& st) const {
  std::string d;
  auto add = [&](const std::string& s) { d += (d.empty() ? "" : " ") + s; };
  const bool in_k = st.kernel == Kernel::Rows28 || st.kernel == Kernel::Conv1x1Cat;  // no activation written
  if (st.ds_op >= 0) add((in_k ? "dsk=" : "ds=") + ops_[st.ds_op].name);
  if (st.pool_op >= 0) add("pool=" + ops_[st.pool_op].name);
  if (st.src_op >= 0) add("in=" + ops_[st.src_op].name);
  if (st.wreg) add("wreg");
  if (!st.store_y) add("nostore");
  if (st.side) add("side");
  if (st.cfg >= 0) add("cfg=" + std::to_string(st.cfg));
  if (st.count > 0) {
    const char* what = st.kernel == Kernel::Small ? "mf=" : st.kernel == Kernel::SoftmaxTopK ? "k=" : st.kernel == Kernel::Embed ? "hw=" : (st.kernel == Kernel::BigTile || st.kernel == Kernel::FcGemm) ? "splits=" : "strip=";
    add(what + std::to_string(st.count));
  }
  return d;
}

std::vector<Engine::PlanLine> Engine::plan_lines(const std::vector<Step>& steps) const {
  std::vector<PlanLine> out;
  for (const Step& st : steps) out.push_back(PlanLine{kernel_name(st.kernel), ops_[st.first_op].name, step_detail(st), st.n_ops});
  return out;
}

std::vector<Engine::PlanLine> Engine::plan_audit(const std::string& arch, const WeightMap& weights,
                                                 const EngineOptions& options, const PlanSpec& spec, int num_cus,
                                                 std::vector<Op>* engine_ops, int num_classes, int image_size) {
  Engine e(HostOnly{}, arch, weights, num_classes, image_size, options);
  e.num_cus_ = num_cus;
  e.layout_weights();
  if (engine_ops) *engine_ops = e.ops_;
  return e.plan_lines(e.plan(spec));
}

}  // namespace dmlc
