// GPU inference engine implementation (see engine.h).
//
// Model definitions follow the torchvision/tch-rs layer naming that the
// reference's `.ot` checkpoints use (tch::vision::resnet::resnet18 and
// tch::vision::alexnet::alexnet, constructed at src/services.rs:515,521):
// conv1/bn1/layer{1..4}.{i}.{conv,bn}{1,2[,3]}/downsample.{0,1}/fc and
// features.{0,3,6,8,10}/classifier.{1,4,6}.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <optional>
#include <stdexcept>

#include "trace.h"

namespace dmlc {

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

const HostTensor& need(const WeightMap& w, const std::string& k) {
  auto it = w.find(k);
  if (it == w.end()) throw std::runtime_error("missing weight: " + k);
  return it->second;
}

const HostTensor* maybe(const WeightMap& w, const std::string& k) {
  auto it = w.find(k);
  return it == w.end() ? nullptr : &it->second;
}

uint16_t f2bf_host(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;  // NaN
  u += 0x7fffu + ((u >> 16) & 1u);                        // round to nearest even
  return (uint16_t)(u >> 16);
}

float bf2f_host(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// float -> OCP e4m3 (bias 7, max 448, no infinities), round to nearest even,
// saturating; exact by search over the 127 non-negative finite codes.
uint8_t f2e4m3_host(float f) {
  static const std::vector<float> table = [] {
    std::vector<float> t(127);
    for (int c = 0; c < 127; ++c) {
      const int e = c >> 3, m = c & 7;
      t[c] = e == 0 ? std::ldexp((float)m / 8.f, -6) : std::ldexp(1.f + (float)m / 8.f, e - 7);
    }
    return t;
  }();
  if (std::isnan(f)) return 0x7f;
  const uint8_t sign = std::signbit(f) ? 0x80 : 0;
  const float a = std::fabs(f);
  if (a >= 448.f) return sign | 0x7e;
  int c = (int)(std::upper_bound(table.begin(), table.end(), a) - table.begin()) - 1;  // table[c] <= a
  if (c < 126) {
    const float lo = table[c], hi = table[c + 1];
    if (a - lo > hi - a || (a - lo == hi - a && (c & 1))) ++c;
  }
  return sign | (uint8_t)c;
}

}  // namespace

bool EngineOptions::set(const std::string& name, bool v) {
  static const std::pair<const char*, bool EngineOptions::*> fields[] = {
      {"persistent", &EngineOptions::persistent},   {"fused_stem", &EngineOptions::fused_stem},
      {"fused_preprocess", &EngineOptions::fused_preprocess}, {"row_conv", &EngineOptions::row_conv},
      {"rows_wreg", &EngineOptions::rows_wreg},     {"fused_block", &EngineOptions::fused_block},
      {"fused_bottleneck", &EngineOptions::fused_bottleneck},
      {"ds_into_expand", &EngineOptions::ds_into_expand}, {"ds_into_conv2", &EngineOptions::ds_into_conv2},
      {"chain_1x1", &EngineOptions::chain_1x1},
      {"fp8_3x3_in", &EngineOptions::fp8_3x3_in},
      {"stream_conv", &EngineOptions::stream_conv}, {"stream_wreg", &EngineOptions::stream_wreg},
      {"stream_l4s2", &EngineOptions::stream_l4s2}, {"fuse_ds", &EngineOptions::fuse_ds},
      {"bigtile", &EngineOptions::bigtile},         {"fused_pool", &EngineOptions::fused_pool},
      {"fused_head", &EngineOptions::fused_head},   {"fc_small", &EngineOptions::fc_small},
      {"direct13", &EngineOptions::direct13},
      {"direct27", &EngineOptions::direct27},
      {"fork_ds", &EngineOptions::fork_ds},         {"fp8_3x3", &EngineOptions::fp8_3x3},
      {"fp8_3x3_out", &EngineOptions::fp8_3x3_out},
      {"fp8_3x3_out_s2", &EngineOptions::fp8_3x3_out_s2},
      {"conv1x1", &EngineOptions::conv1x1},         {"s2rows", &EngineOptions::s2rows},
      {"s2rows128", &EngineOptions::s2rows128},
      {"rows28", &EngineOptions::rows28},           {"stem_roles", &EngineOptions::stem_roles},
      {"stem_dense", &EngineOptions::stem_dense},
      {"fc_gemm", &EngineOptions::fc_gemm},
      {"igemm_small_m", &EngineOptions::igemm_small_m},
      {"small_conv", &EngineOptions::small_conv},
  };
  for (const auto& f : fields)
    if (name == f.first) {
      this->*(f.second) = v;
      return true;
    }
  return false;
}

Engine::Engine(const std::string& arch, const WeightMap& weights, int device, int num_classes,
               int image_size, const EngineOptions& options)
    : arch_(arch), device_(device), num_classes_(num_classes), image_size_(image_size), opt_(options) {
  if (num_classes % 4 != 0) throw std::invalid_argument("num_classes must be a multiple of 4");
  DMLC_HIP_CHECK(hipSetDevice(device_));
  hipDeviceProp_t prop;
  DMLC_HIP_CHECK(hipGetDeviceProperties(&prop, device_));
  num_cus_ = prop.multiProcessorCount;
  build_graph(weights, true);
  pack_weights(weights);
  init_device();
}

Engine::Engine(HostOnly, const std::string& arch, const WeightMap& weights, int num_classes, int image_size,
               const EngineOptions& options)
    : arch_(arch), device_(-1), num_classes_(num_classes), image_size_(image_size), opt_(options) {
  if (num_classes % 4 != 0) throw std::invalid_argument("num_classes must be a multiple of 4");
  build_graph(weights, false);
}

void Engine::build_graph(const WeightMap& weights, bool calibrate_on_device) {
  if (arch_ == "resnet18")
    build_resnet({2, 2, 2, 2}, false);
  else if (arch_ == "resnet34")
    build_resnet({3, 4, 6, 3}, false);
  else if (arch_ == "resnet50")
    build_resnet({3, 4, 6, 3}, true);
  else if (arch_ == "resnet50_fp8") {
    fp8_ = true;
    build_resnet({3, 4, 6, 3}, true);
    mark_fp8();
    if (calibrate_on_device) {
      calibrate(weights);
    } else {  // host-only audit: unit scales, same layout
      for (size_t i = 0; i < shapes_.size(); ++i)
        if (shapes_[i].fp8 && chan_act_[i]) shapes_[i].cscale.assign(shapes_[i].C, 1.f);
    }
  }
  else if (arch_ == "alexnet")
    build_alexnet();
  else
    throw std::invalid_argument("unknown arch: " + arch_);
}

std::vector<PackRegion> Engine::pack_audit(const std::string& arch, const WeightMap& weights,
                                           const EngineOptions& options, size_t* total, int num_classes,
                                           int image_size) {
  Engine e(HostOnly{}, arch, weights, num_classes, image_size, options);
  std::vector<PackRegion> regions;
  const std::vector<uint8_t> host = e.pack_host(weights, &regions);
  if (total) *total = host.size();
  return regions;
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

// Same graph, packing and calibration as `src`, on another device, with an
// uninitialised weight arena: the caller fills it (an RCCL broadcast of the
// source arena, GpuExecutor::ModelSlot). The host packing runs once per model
// instead of once per GPU.
Engine::Engine(const Engine& src, int device)
    : arch_(src.arch_), device_(device), num_classes_(src.num_classes_), image_size_(src.image_size_) {
  DMLC_HIP_CHECK(hipSetDevice(device_));
  hipDeviceProp_t prop;
  DMLC_HIP_CHECK(hipGetDeviceProperties(&prop, device_));
  num_cus_ = prop.multiProcessorCount;
  stem_pad_ = src.stem_pad_;
  opt_ = src.opt_;
  fp8_ = src.fp8_;
  shapes_ = src.shapes_;
  convs_ = src.convs_;
  ops_ = src.ops_;
  logits_act_ = src.logits_act_;
  weight_bytes_ = src.weight_bytes_;
  DMLC_HIP_CHECK(hipMalloc(&warena_, weight_bytes_));
  init_device();
}

void Engine::copy_weights_from(const Engine& src) {
  if (src.device_ != device_ || src.weight_bytes_ != weight_bytes_ || src.arch_ != arch_)
    throw std::invalid_argument("Engine::copy_weights_from: not a same-device replica");
  DMLC_HIP_CHECK(hipSetDevice(device_));
  DMLC_HIP_CHECK(hipMemcpy(warena_, src.warena_, weight_bytes_, hipMemcpyDeviceToDevice));
}

void Engine::init_device() {
  DMLC_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  DMLC_HIP_CHECK(hipEventCreateWithFlags(&ev_out_, hipEventDisableTiming));
  DMLC_HIP_CHECK(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking));
  fork_evs_.resize(ops_.size());
  join_evs_.resize(ops_.size());
  for (size_t i = 0; i < ops_.size(); ++i) {
    DMLC_HIP_CHECK(hipEventCreateWithFlags(&fork_evs_[i], hipEventDisableTiming));
    DMLC_HIP_CHECK(hipEventCreateWithFlags(&join_evs_[i], hipEventDisableTiming));
  }
  DMLC_HIP_CHECK(hipMalloc(&ws_, kSplitKWsElems * sizeof(float)));
  DMLC_HIP_CHECK(hipMalloc(&zero_, 256));
  DMLC_HIP_CHECK(hipMemset(zero_, 0, 256));
}

Engine::~Engine() {
  if (device_ < 0) return;  // host-only (pack_audit): nothing on a device
  hipSetDevice(device_);
  for (auto& kv : graphs_) hipGraphExecDestroy(kv.second);
  if (!acts_.empty() && acts_[0]) hipFree(acts_[0]);
  if (warena_) hipFree(warena_);
  if (ws_) hipFree(ws_);
  if (bt_ws_) hipFree(bt_ws_);
  if (zero_) hipFree(zero_);
  if (dummy_idx_) hipFree(dummy_idx_);
  if (head_ws_) hipFree(head_ws_);
  if (ev_out_) hipEventDestroy(ev_out_);
  for (auto e : fork_evs_) hipEventDestroy(e);
  for (auto e : join_evs_) hipEventDestroy(e);
  if (side_) hipStreamDestroy(side_);
  if (stream_) hipStreamDestroy(stream_);
}

int Engine::add_act(ActShape s) {
  shapes_.push_back(s);
  return (int)shapes_.size() - 1;
}

int Engine::op_count_conv() const { return (int)convs_.size(); }

int Engine::conv(int in, const std::string& name, const std::string& bn, int cout, int k,
                 int stride, int pad, bool relu, int res) {
  const ActShape is = shapes_.at(in);
  ConvLayer L;
  L.name = name;
  L.bn = bn;
  L.pair = (op_count_conv() == 0 && is.C == 3);  // stem reads the packed RGB image
  L.cin_eff = is.C;
  L.cin = is.C;
  L.cout = cout;
  L.kh = L.kw = k;
  L.stride = stride;
  L.pad = pad;
  L.relu = relu;
  convs_.push_back(L);
  ActShape os{conv_out_dim(is.H, k, stride, pad), conv_out_dim(is.W, k, stride, pad), cout, false};
  if (L.pair) {  // stem: padding is in the image; its rows are wider than S + 2p
    os.H = conv_out_dim(image_size_, k, stride, stem_pad_);
    os.W = os.H;
  }
  convs_.back().in_act = in;
  const int out = add_act(os);
  convs_.back().out_act = out;
  Op op{OpType::Conv, in, out, res, (int)convs_.size() - 1, 0, 0, 0, name};
  ops_.push_back(op);
  return out;
}

int Engine::fc(int in, const std::string& name, int cout, bool relu, bool last) {
  const ActShape is = shapes_.at(in);
  ConvLayer L;
  L.name = name;
  L.fc = true;
  L.cin = L.cin_eff = is.H * is.W * is.C;
  if (is.H * is.W > 1) {
    L.fc_hwc[0] = is.H;
    L.fc_hwc[1] = is.W;
    L.fc_hwc[2] = is.C;
  }
  L.cout = cout;
  L.relu = relu;
  convs_.push_back(L);
  const int out = add_act(ActShape{1, 1, cout, last});
  ops_.push_back(Op{OpType::Conv, in, out, -1, (int)convs_.size() - 1, 0, 0, 0, name});
  return out;
}

void Engine::build_resnet(const std::vector<int>& blocks, bool bottleneck) {
  const int S = image_size_;
  stem_pad_ = 3;  // packed RGB image with the 7x7/s2 stem's padding built in
  int x;
  if (opt_.fused_stem && S % 32 == 0 && S >= 128 && S <= 256) {
    // paired image -> one kernel for conv1 + bn1 + relu + maxpool
    const int pairs = stem_row_width(S, 3, 7, 2) / 2;
    x = add_act(ActShape{S + 6, pairs, 8, false});
    ops_.push_back(Op{OpType::Preprocess, -1, x, -1, -1, 1, 0, 3, "preprocess"});
    ConvLayer L;
    L.name = "conv1";
    L.bn = "bn1";
    L.stem_pool = true;
    L.cin = L.cin_eff = 3;
    L.cout = 64;
    L.kh = L.kw = 7;
    L.stride = 2;
    L.pad = 3;
    L.relu = true;
    convs_.push_back(L);
    const int y = add_act(ActShape{S / 4, S / 4, 64, false});
    ops_.push_back(Op{OpType::StemPool, x, y, -1, (int)convs_.size() - 1, 0, 0, 0, "conv1+maxpool"});
    x = y;
  } else {
    x = add_act(ActShape{S + 6, stem_row_width(S, 3, 7, 2), 3, false});
    ops_.push_back(Op{OpType::Preprocess, -1, x, -1, -1, 0, 0, 3, "preprocess"});
    x = conv(x, "conv1", "bn1", 64, 7, 2, 0, true);
    const ActShape s = shapes_[x];
    const int y = add_act(ActShape{conv_out_dim(s.H, 3, 2, 1), conv_out_dim(s.W, 3, 2, 1), s.C, false});
    ops_.push_back(Op{OpType::MaxPool, x, y, -1, -1, 3, 2, 1, "maxpool"});
    x = y;
  }
  int inplanes = 64;
  for (int li = 0; li < 4; ++li) {
    const int planes = 64 << li;
    for (int bi = 0; bi < blocks[li]; ++bi) {
      const int stride = (li > 0 && bi == 0) ? 2 : 1;
      const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(bi);
      const int outp = bottleneck ? planes * 4 : planes;
      int identity = x;
      if (stride != 1 || inplanes != outp) {
        identity = conv(x, p + ".downsample.0", p + ".downsample.1", outp, 1, stride, 0, false);
        ops_.back().side = true;
      }
      if (!bottleneck) {
        const int y = conv(x, p + ".conv1", p + ".bn1", planes, 3, stride, 1, true);
        x = conv(y, p + ".conv2", p + ".bn2", planes, 3, 1, 1, true, identity);
      } else {
        int y = conv(x, p + ".conv1", p + ".bn1", planes, 1, 1, 0, true);
        y = conv(y, p + ".conv2", p + ".bn2", planes, 3, stride, 1, true);
        x = conv(y, p + ".conv3", p + ".bn3", outp, 1, 1, 0, true, identity);
      }
      inplanes = outp;
    }
  }
  {
    const ActShape s = shapes_[x];
    const int y = add_act(ActShape{1, 1, s.C, false});
    ops_.push_back(Op{OpType::AvgPoolGlobal, x, y, -1, -1, 0, 0, 0, "avgpool"});
    x = y;
  }
  logits_act_ = fc(x, "fc", num_classes_, false, true);
  ops_.push_back(Op{OpType::SoftmaxTop1, logits_act_, -1, -1, -1, 0, 0, 0, "softmax_top1"});
}

void Engine::build_alexnet() {
  const int S = image_size_;
  stem_pad_ = 2;  // packed RGB image with the 11x11/s4 stem's padding built in
  int x = add_act(ActShape{S + 4, stem_row_width(S, 2, 11, 4), 3, false});
  ops_.push_back(Op{OpType::Preprocess, -1, x, -1, -1, 0, 0, 2, "preprocess"});
  auto pool = [&](int in, const std::string& n) {
    const ActShape s = shapes_[in];
    const int y = add_act(ActShape{conv_out_dim(s.H, 3, 2, 0), conv_out_dim(s.W, 3, 2, 0), s.C, false});
    ops_.push_back(Op{OpType::MaxPool, in, y, -1, -1, 3, 2, 0, n});
    return y;
  };
  x = conv(x, "features.0", "", 64, 11, 4, 0, true);
  // 224x224 u8 batches skip preprocess + features.0 + features.2: one fused
  // kernel (alex_stem.hip) writes features.2's output
  convs_.back().alex_stem = opt_.fused_stem && alex_stem_supported(S);
  x = pool(x, "features.2");
  x = conv(x, "features.3", "", 192, 5, 1, 2, true);
  x = pool(x, "features.5");
  x = conv(x, "features.6", "", 384, 3, 1, 1, true);
  x = conv(x, "features.8", "", 256, 3, 1, 1, true);
  x = conv(x, "features.10", "", 256, 3, 1, 1, true);
  x = pool(x, "features.12");
  {
    const ActShape s = shapes_[x];
    if (!(s.H == 6 && s.W == 6)) {
      const int y = add_act(ActShape{6, 6, s.C, false});
      ops_.push_back(Op{OpType::AvgPoolAdaptive, x, y, -1, -1, 0, 0, 0, "avgpool"});
      x = y;
    }
  }
  x = fc(x, "classifier.1", 4096, true, false);
  x = fc(x, "classifier.4", 4096, true, false);
  logits_act_ = fc(x, "classifier.6", num_classes_, false, true);
  ops_.push_back(Op{OpType::SoftmaxTop1, logits_act_, -1, -1, -1, 0, 0, 0, "softmax_top1"});
}

// resnet50_fp8: conv outputs with a multiple of 128 channels are e4m3: the
// 256..2048-channel block outputs and residual paths (where the bytes are:
// layer1's 56x56x256 tensors dominate the traffic), so every 1x1 expand /
// reduce conv and downsample reads or writes e4m3. The bottleneck 3x3 convs
// of layers 2-4 then read e4m3 too and run on the e4m3 MFMA
// (conv3x3_stream8.hip, fp8_3x3_in: their t1 gets per-channel scales from the
// reduce 1x1) and write e4m3 (fp8_3x3_out), so the expand convs read e4m3.
// (EngineOptions::fp8_3x3 instead marks every 3x3 conv's input and output
// e4m3 for the fp8 implicit GEMM: slower, off.) The stem and layer1's
// 64-channel inner convs stay bf16 (Cin = 64 is below the fp8 kernels'
// 128-channel K-tile).
void Engine::mark_fp8() {
  const bool fp8_3x3 = opt_.fp8_3x3;
  std::vector<bool> near_3x3(shapes_.size(), false);  // read or written by a 3x3 conv
  for (const Op& op : ops_)
    if (op.type == OpType::Conv && !convs_[op.conv].fc && convs_[op.conv].kh == 3) {
      near_3x3[op.in] = true;
      near_3x3[op.out] = true;
    }
  for (const Op& op : ops_)
    if (op.type == OpType::Conv && !convs_[op.conv].fc && shapes_[op.out].C % 128 == 0 &&
        (fp8_3x3 || !near_3x3[op.out]))
      shapes_[op.out].fp8 = true;
  chan_act_.assign(shapes_.size(), false);
  if (opt_.fp8_3x3_out && !fp8_3x3) {
    // outputs of 3x3 convs that no 3x3 conv reads (a bottleneck's t2), where
    // the conv runs on conv3x3_rows28 / conv3x3_stream (e4m3 epilogues)
    std::vector<bool> in_3x3(shapes_.size(), false);
    for (const Op& op : ops_)
      if (op.type == OpType::Conv && !convs_[op.conv].fc && convs_[op.conv].kh == 3) in_3x3[op.in] = true;
    for (const Op& op : ops_) {
      if (op.type != OpType::Conv) continue;
      const ConvLayer& L = convs_[op.conv];
      const ActShape& is = shapes_[op.in];
      if (L.fc || L.kh != 3 || L.kw != 3 || L.pad != 1 || op.res >= 0 || in_3x3[op.out] ||
          shapes_[op.out].C % 128 || shapes_[op.in].fp8)
        continue;
      if (conv3x3_rows28_supported(is.H, is.W, is.C, L.cout) ||
          conv3x3_stream_supported(is.H, is.W, is.C, L.cout, L.stride) || (opt_.fp8_3x3_out_s2 && L.stride == 2)) {
        shapes_[op.out].fp8 = true;
        chan_act_[op.out] = true;
      }
    }
    if (opt_.fp8_3x3_in) {
      // ... and their e4m3 input t1 where the e4m3 3x3 kernel runs the conv:
      // t1 is written by a 1x1 conv and read by nothing else
      for (const Op& op : ops_) {
        if (op.type != OpType::Conv) continue;
        const ConvLayer& L = convs_[op.conv];
        const ActShape& is = shapes_[op.in];
        if (L.fc || L.kh != 3 || L.kw != 3 || L.pad != 1 || op.res >= 0 || is.fp8 || is.f32 ||
            shapes_[op.out].f32 || in_3x3[op.out] || !conv3x3_stream8_supported(is.H, is.W, is.C, L.cout, L.stride))
          continue;
        if (!chan_act_[op.out] && (L.stride == 1 || shapes_[op.out].fp8)) continue;
        int producers = 0, readers = 0;
        bool from_1x1 = false;
        for (const Op& o : ops_) {
          if (o.type == OpType::Conv && o.out == op.in) {
            ++producers;
            const ConvLayer& P = convs_[o.conv];
            from_1x1 = !P.fc && P.kh == 1 && P.kw == 1 && P.stride == 1 && o.res < 0;
          }
          if (o.in == op.in || o.res == op.in) ++readers;
        }
        if (producers != 1 || !from_1x1 || readers != 1) continue;
        shapes_[op.in].fp8 = true;
        chan_act_[op.in] = true;
        // (a strided one's t2: e4m3 out too, per-channel scales, as the stride-1 ones')
        shapes_[op.out].fp8 = true;
        chan_act_[op.out] = true;
      }
    }
  }
  for (const Op& op : ops_) {
    if (op.type != OpType::Conv) continue;
    if (op.res >= 0 && shapes_[op.res].fp8 != shapes_[op.out].fp8)
      throw std::runtime_error("mark_fp8: residual and output dtypes differ at " + op.name);
    if (shapes_[op.in].fp8 && shapes_[op.in].C % 128)
      throw std::runtime_error("mark_fp8: fp8 conv needs Cin % 128 == 0: " + op.name);
  }
}

// Static per-tensor activation scales: run the bf16 model on a synthetic
// calibration batch and take amax/448 of every tensor that is stored as e4m3.
void Engine::calibrate(const WeightMap& w) {
  const int Bc = 8;
  // every activation must be materialised: no path that computes one inside
  // its reader (the layer1.0 downsample inside the expand conv)
  EngineOptions ro;
  ro.ds_into_expand = false;
  ro.fused_bottleneck = false;
  Engine ref(arch_.substr(0, arch_.find("_fp8")), w, device_, num_classes_, image_size_, ro);
  if (ref.num_activations() != num_activations()) throw std::runtime_error("calibrate: graph mismatch");
  ref.reserve(Bc);
  const size_t img_bytes = (size_t)Bc * image_size_ * image_size_ * 3;
  std::vector<uint8_t> host(img_bytes);
  uint32_t st = 12345u;  // fixed-seed xorshift: deterministic scales
  for (auto& v : host) {
    st ^= st << 13;
    st ^= st >> 17;
    st ^= st << 5;
    v = (uint8_t)(st >> 24);
  }
  uint8_t* d_img = nullptr;
  DMLC_HIP_CHECK(hipMalloc(&d_img, img_bytes));
  DMLC_HIP_CHECK(hipMemcpy(d_img, host.data(), img_bytes, hipMemcpyHostToDevice));
  ref.forward(d_img, Bc, image_size_, image_size_, nullptr, nullptr, nullptr, nullptr, false);
  DMLC_HIP_CHECK(hipDeviceSynchronize());
  DMLC_HIP_CHECK(hipFree(d_img));
  for (int i = 0; i < num_activations(); ++i) {
    if (!shapes_[i].fp8) continue;
    const size_t n = shapes_[i].elems_per_image() * Bc;
    std::vector<uint16_t> a(n);
    DMLC_HIP_CHECK(hipMemcpy(a.data(), ref.activation(i), n * 2, hipMemcpyDeviceToHost));
    float amax = 0.f;
    for (uint16_t v : a) amax = std::max(amax, std::fabs(bf2f_host(v)));
    shapes_[i].scale = std::max(amax, 1e-6f) / 448.f;
    if (!chan_act_[i]) continue;
    // per-channel scales (a channel whose calibration values stay tiny gets
    // 1/1000 of the tensor's range instead of an unbounded 1 / scale)
    const int C = shapes_[i].C;
    std::vector<float> cm(C, 0.f);
    for (size_t j = 0; j < n; ++j) cm[j % C] = std::max(cm[j % C], std::fabs(bf2f_host(a[j])));
    shapes_[i].cscale.resize(C);
    for (int c = 0; c < C; ++c) shapes_[i].cscale[c] = std::max(cm[c], std::max(amax, 1e-6f) * 1e-3f) / 448.f;
    shapes_[i].scale = 1.f;
  }
}

namespace {

// A layer's region of the host weight image: every write is bounds-checked
// against the size the layout pass gave it, so a packing order that writes
// past its region fails at load instead of corrupting its neighbours.
struct RegionRef {
  uint8_t* base = nullptr;
  size_t bytes = 0;
  const std::string* layer = nullptr;
  const char* kind = "";
  template <class T>
  T& at(size_t i) const {
    if ((i + 1) * sizeof(T) > bytes)
      throw std::runtime_error("pack_weights: write past the " + std::string(kind) + " region of " + *layer);
    return reinterpret_cast<T*>(base)[i];
  }
  void copy(size_t off, const void* src, size_t n) const {
    if (off + n > bytes)
      throw std::runtime_error("pack_weights: copy past the " + std::string(kind) + " region of " + *layer);
    std::memcpy(base + off, src, n);
  }
};

}  // namespace

void Engine::pack_weights(const WeightMap& w) {
  const std::vector<uint8_t> host = pack_host(w, nullptr);
  DMLC_HIP_CHECK(hipMalloc(&warena_, weight_bytes_));
  DMLC_HIP_CHECK(hipMemcpy(warena_, host.data(), weight_bytes_, hipMemcpyHostToDevice));
}

// Layout pass: every layer's padded sizes and the offsets of its regions in
// the weight arena (all the planner reads of the packing).
void Engine::layout_weights() {
  size_t off = 0;
  for (auto& L : convs_) {
    L.npad = conv_npad(L.cout);
    L.kpad = L.stem_pool ? kStemPoolK : conv_kpad(L.cin_eff, L.kh, L.kw, L.pair);
    L.fp8 = L.in_act >= 0 && shapes_[L.in_act].fp8;
    L.w_off = off;
    off = align_up(off + (size_t)L.npad * L.kpad * (L.fp8 ? 1 : 2), 256);
    L.b_off = off;
    off = align_up(off + (size_t)L.npad * 4, 256);
    if (L.fp8) {
      L.a_off = off;
      off = align_up(off + (size_t)L.npad * 4, 256);
    }
    L.wf_off = 0;
    L.wf_bytes = 0;
    // Who gets a bf16 fragment-order copy: the plain 3x3/p1 convs and 1x1/s2
    // downsamples that a kernel reading its weights in that order can run.
    const ActShape is = L.in_act >= 0 ? shapes_[L.in_act] : ActShape{};
    const bool conv_or_ds = (L.plain_3x3() || L.plain_ds2()) && L.cout % 32 == 0;
    // every one the query-batch conv can run (conv_small.hip)
    const bool small = conv_or_ds && conv_small_supported(is.H, is.W, is.C, L.cout, L.stride);
    // the register-weight stream conv with the downsample it fuses next to a
    // stride-2 one, and layer2.0's pair on conv3x3_s2rows
    const bool stream = conv_or_ds && (conv3x3_stream_uses_frag(is.H, is.W, is.C, L.cout, L.stride) ||
                                       (L.stride == 2 && conv3x3_s2rows_supported(is.H, is.W, is.C, L.cout)));
    // the stride-1 row kernels and AlexNet's 13x13 convs
    const bool rows = L.plain_3x3() && L.cout % 32 == 0 && L.stride == 1 &&
                      (conv3x3_rows28_supported(is.H, is.W, is.C, L.cout) ||
                       conv3x3_rows_supported(is.H, is.W, is.C, L.cout) ||
                       conv3x3_13_supported(is.H, is.W, is.C, L.cout));
    if (small || ((stream || rows) && L.kpad % 32 == 0)) {
      L.wf_off = off;
      L.wf_bytes = (size_t)L.cout * L.kpad * 2;
      off = align_up(off + L.wf_bytes, 256);
    }
    if (L.plain() && L.kh == 5 && L.kw == 5 && L.stride == 1 &&
        conv5x5_27_supported(is.H, is.W, is.C, L.cout, L.pad)) {
      L.wf_off = off;  // fragment-order copy for conv_direct.hip
      L.wf_bytes = (size_t)L.cout * L.kpad * 2;
      off = align_up(off + L.wf_bytes, 256);
    }
    if (L.fp8 && !L.fc && L.in_act >= 0 && L.kh == 3 && L.kw == 3 && L.pad == 1 && L.kpad == 9 * L.cin &&
        conv3x3_stream8_supported(is.H, is.W, is.C, L.cout, L.stride)) {
      L.wf_off = off;  // e4m3 fragment-order copy for conv3x3_stream8.hip
      L.wf_bytes = (size_t)L.cout * L.kpad;
      off = align_up(off + L.wf_bytes, 256);
    }
    if (bottleneck_conv3(L)) {  // fragment-order copy for bottleneck56.hip's expand conv
      L.wf_off = off;
      L.wf_bytes = (size_t)L.cout * L.kpad * 2;
      off = align_up(off + L.wf_bytes, 256);
    }
    if (L.stem_pool) {  // dense-K order for the one-image-per-workgroup stem (stem_dense_k_index)
      L.wf_off = off;
      L.wf_bytes = (size_t)L.cout * kStemDenseK * 2;
      off = align_up(off + L.wf_bytes, 256);
    }
    if (L.alex_stem) {  // paired-chunk K order for alex_stem.hip
      L.wf_off = off;
      L.wf_bytes = (size_t)L.cout * kAlexStemK * 2;
      off = align_up(off + L.wf_bytes, 256);
    }
  }
  // bottleneck expand convs that can take their stride-1 downsample as a
  // second K block (conv1x1 with x2): both bf16 in, 1x1, same output
  for (size_t j = 0; j < ops_.size(); ++j) {
    const Op& c3 = ops_[j];
    if (c3.type != OpType::Conv || c3.res < 0) continue;
    ConvLayer& L3 = convs_[c3.conv];
    for (size_t i = 0; i < j; ++i) {
      const Op& d = ops_[i];
      if (d.type != OpType::Conv || d.out != c3.res) continue;
      const ConvLayer& D = convs_[d.conv];
      if (D.fc || L3.fc || D.kh != 1 || D.kw != 1 || D.stride != 1 || D.relu || !L3.relu || L3.kh != 1 ||
          L3.kw != 1 || L3.stride != 1 || D.fp8 || L3.fp8 || shapes_[d.in].fp8 || shapes_[c3.in].fp8 ||
          D.cout != L3.cout || D.npad != L3.npad || shapes_[d.in].H != shapes_[c3.in].H ||
          shapes_[d.in].W != shapes_[c3.in].W || D.kpad != D.cin || L3.kpad != L3.cin)
        continue;
      L3.cat_ds = d.conv;
      L3.cat_off = off;
      off = align_up(off + (size_t)L3.npad * (L3.kpad + D.kpad) * 2, 256);
      L3.cat_b_off = off;
      off = align_up(off + (size_t)L3.npad * 4, 256);
    }
  }
  weight_bytes_ = off;
}

std::vector<uint8_t> Engine::pack_host(const WeightMap& w, std::vector<PackRegion>* regions) {
  layout_weights();
  std::vector<uint8_t> host(weight_bytes_, 0);
  auto region = [&](const ConvLayer& L, const char* kind, size_t roff, size_t bytes) {
    if (roff + bytes > host.size())
      throw std::runtime_error("pack_weights: " + std::string(kind) + " region of " + L.name + " past the arena");
    if (regions) regions->push_back(PackRegion{L.name, kind, roff, bytes});
    return RegionRef{host.data() + roff, bytes, &L.name, kind};
  };
  for (auto& L : convs_) {
    const HostTensor& W = need(w, L.name + ".weight");
    const HostTensor* cb = maybe(w, L.name + ".bias");
    std::vector<float> scale(L.cout, 1.f), bias(L.cout, 0.f);
    if (cb) {
      if (cb->numel() != L.cout) throw std::runtime_error("bad bias size: " + L.name);
      for (int n = 0; n < L.cout; ++n) bias[n] = cb->data[n];
    }
    if (!L.bn.empty()) {
      const HostTensor& g = need(w, L.bn + ".weight");
      const HostTensor& b = need(w, L.bn + ".bias");
      const HostTensor& m = need(w, L.bn + ".running_mean");
      const HostTensor& v = need(w, L.bn + ".running_var");
      for (int n = 0; n < L.cout; ++n) {
        const double s = (double)g.data[n] / std::sqrt((double)v.data[n] + 1e-5);
        scale[n] = (float)s;
        bias[n] = (float)((double)b.data[n] + ((double)bias[n] - (double)m.data[n]) * s);
      }
    }
    if (L.out_act >= 0 && !shapes_[L.out_act].cscale.empty()) {
      // the conv writes e4m3 with per-channel scales: fold 1 / cscale[n] into
      // its weights and bias (ReLU commutes with a positive scale)
      const std::vector<float>& cs = shapes_[L.out_act].cscale;
      for (int n = 0; n < L.cout; ++n) {
        scale[n] /= cs[n];
        bias[n] /= cs[n];
      }
    }
    const RegionRef rw = region(L, "w", L.w_off, (size_t)L.npad * L.kpad * (L.fp8 ? 1 : 2));
    const RegionRef rb = region(L, "b", L.b_off, (size_t)L.npad * 4);
    const RegionRef rf = L.wf_off ? region(L, "wf", L.wf_off, L.wf_bytes) : RegionRef{};
    std::vector<uint16_t> wbf;
    RegionRef rwbf = rw;  // bf16 weights [npad][kpad]
    if (L.fp8) {  // fold into a bf16 staging copy first, then quantise per row
      wbf.assign((size_t)L.npad * L.kpad, 0);
      rwbf.base = (uint8_t*)wbf.data();
      rwbf.bytes = wbf.size() * 2;
      rwbf.kind = "bf16 staging";
    }
    auto pw = [&](size_t i) -> uint16_t& { return rwbf.at<uint16_t>(i); };
    if (!L.fc) {
      if (W.shape.size() != 4 || W.shape[0] != L.cout || W.shape[1] != L.cin || W.shape[2] != L.kh ||
          W.shape[3] != L.kw)
        throw std::runtime_error("bad conv weight shape: " + L.name);
      for (int n = 0; n < L.cout; ++n)
        for (int c = 0; c < L.cin; ++c)
          for (int i = 0; i < L.kh; ++i)
            for (int j = 0; j < L.kw; ++j) {
              const float v = W.data[(((size_t)n * L.cin + c) * L.kh + i) * L.kw + j] * scale[n];
              size_t k;
              if (L.stem_pool)  // paired stem: chunk (kw/2) of row kh, slot 3*(kw%2) + c
                k = (size_t)i * 32 + (j / 2) * 8 + (j % 2) * 3 + c;
              else if (L.pair)  // stem: k = kh*CPK*8 + kw*3 + c
                k = (size_t)i * ((L.kw * 3 + 7) / 8) * 8 + j * 3 + c;
              else
                k = (size_t)(i * L.kw + j) * L.cin_eff + c;
              pw((size_t)n * L.kpad + k) = f2bf_host(v);
            }
    } else {
      if (W.shape.size() != 2 || W.shape[0] != L.cout || W.shape[1] != L.cin)
        throw std::runtime_error("bad linear weight shape: " + L.name);
      const int H = L.fc_hwc[0], Wd = L.fc_hwc[1], C = L.fc_hwc[2];
      for (int n = 0; n < L.cout; ++n)
        for (int k = 0; k < L.cin; ++k) {
          int dst = k;
          if (H > 0) {  // torch flattens NCHW (c,h,w); our activations are NHWC (h,w,c)
            const int c = k / (H * Wd), hw = k % (H * Wd);
            dst = hw * C + c;
          }
          pw((size_t)n * L.kpad + dst) = f2bf_host(W.data[(size_t)n * L.cin + k] * scale[n]);
        }
    }
    for (int n = 0; n < L.cout; ++n) rb.at<float>(n) = bias[n];
    if (L.stem_pool) {
      for (int n = 0; n < L.cout; ++n)
        for (int c = 0; c < L.cin; ++c)
          for (int i = 0; i < L.kh; ++i)
            for (int j = 0; j < L.kw; ++j)
              rf.at<uint16_t>((size_t)n * kStemDenseK + stem_dense_k_index(i, j, c)) =
                  f2bf_host(W.data[(((size_t)n * L.cin + c) * L.kh + i) * L.kw + j] * scale[n]);
    } else if (L.alex_stem) {
      for (int n = 0; n < L.cout; ++n)
        for (int c = 0; c < L.cin; ++c)
          for (int i = 0; i < L.kh; ++i)
            for (int j = 0; j < L.kw; ++j)
              rf.at<uint16_t>((size_t)n * kAlexStemK + alex_stem_k(i, j, c)) =
                  f2bf_host(W.data[(((size_t)n * L.cin + c) * L.kh + i) * L.kw + j] * scale[n]);
    } else if (L.wf_off && !L.fp8) {  // bf16 fragment order (e4m3 layers: stream8's order, below)
      for (int n = 0; n < L.cout; ++n)
        for (int k = 0; k < L.kpad; ++k) rf.at<uint16_t>(stream_frag_index(n, k, L.kpad)) = pw((size_t)n * L.kpad + k);
    }
    if (L.fp8) {
      // e4m3 weights with a per-output-channel scale; alpha = s_in * s_w[n]
      const RegionRef& q = rw;
      const RegionRef alpha = region(L, "alpha", L.a_off, (size_t)L.npad * 4);
      const float s_in = shapes_[L.in_act].scale;
      // per-channel input scales (fp8_3x3_out): along K (channel k % Cin)
      const std::vector<float>& ics = shapes_[L.in_act].cscale;
      const int cin = shapes_[L.in_act].C;
      auto wv = [&](int n, int k) {
        const float v = bf2f_host(pw((size_t)n * L.kpad + k));
        return ics.empty() ? v : v * ics[k % cin];
      };
      for (int n = 0; n < L.npad; ++n) {
        float amax = 0.f;
        for (int k = 0; k < L.kpad; ++k) amax = std::max(amax, std::fabs(wv(n, k)));
        const float sw = amax > 0.f ? amax / 448.f : 1.f;
        for (int k = 0; k < L.kpad; ++k) q.at<uint8_t>((size_t)n * L.kpad + k) = f2e4m3_host(wv(n, k) / sw);
        alpha.at<float>(n) = s_in * sw;
      }
      if (L.wf_off) {  // conv3x3_stream8's fragment order of the e4m3 weights
        const uint8_t* qb = q.base;
        const int KT = L.kpad / 128;
        for (int j = 0; j < L.cout / 32; ++j)
          for (int t = 0; t < KT; ++t)
            for (int nf = 0; nf < 2; ++nf)
              for (int h = 0; h < 2; ++h)
                for (int ln = 0; ln < 64; ++ln) {
                  const int fq = ln >> 4, r = 16 * nf + (ln & 15);
                  const int n = 32 * j + 8 * ((r & 15) >> 2) + 4 * (r >> 4) + (r & 3);  // perm32
                  const int k0 = 128 * t + 32 * fq + 16 * (h ^ (fq & 1));
                  rf.copy(conv3x3_stream8_frag_offset(j, t, nf, h, ln, KT), qb + (size_t)n * L.kpad + k0, 16);
                }
      }
    }
  }
  for (auto& L : convs_) {  // [W3 | Wd] and b3 + bd from the folded bf16 copies above
    if (L.cat_ds < 0) continue;
    const ConvLayer& D = convs_[L.cat_ds];
    const int K = L.kpad + D.kpad;
    const RegionRef cw = region(L, "cat", L.cat_off, (size_t)L.npad * K * 2);
    const uint16_t* w3 = (const uint16_t*)(host.data() + L.w_off);
    const uint16_t* wd = (const uint16_t*)(host.data() + D.w_off);
    for (int n = 0; n < L.npad; ++n) {
      cw.copy((size_t)n * K * 2, w3 + (size_t)n * L.kpad, (size_t)L.kpad * 2);
      cw.copy(((size_t)n * K + L.kpad) * 2, wd + (size_t)n * D.kpad, (size_t)D.kpad * 2);
    }
    const RegionRef cb = region(L, "cat_b", L.cat_b_off, (size_t)L.npad * 4);
    const float* b3 = (const float*)(host.data() + L.b_off);
    const float* bd = (const float*)(host.data() + D.b_off);
    for (int n = 0; n < L.npad; ++n) cb.at<float>(n) = b3[n] + bd[n];
  }
  return host;
}

void Engine::reserve(int max_batch) {
  if (max_batch <= max_batch_) return;
  DMLC_HIP_CHECK(hipSetDevice(device_));
  DMLC_HIP_CHECK(hipDeviceSynchronize());
  for (auto& kv : graphs_) hipGraphExecDestroy(kv.second);
  graphs_.clear();
  if (!acts_.empty() && acts_[0]) DMLC_HIP_CHECK(hipFree(acts_[0]));
  if (dummy_idx_) DMLC_HIP_CHECK(hipFree(dummy_idx_));
  std::vector<size_t> offs;
  size_t total = 0;
  for (const auto& s : shapes_) {
    offs.push_back(total);
    total = align_up(total + s.elems_per_image() * max_batch * s.elem_bytes(), 256);
  }
  void* base = nullptr;
  DMLC_HIP_CHECK(hipMalloc(&base, total));
  acts_.clear();
  for (size_t o : offs) acts_.push_back((uint8_t*)base + o);
  act_bytes_ = total;
  DMLC_HIP_CHECK(hipMalloc(&dummy_idx_, (size_t)max_batch * 8));
  max_batch_ = max_batch;
  if (head_ws_) DMLC_HIP_CHECK(hipFree(head_ws_));
  head_ws_bytes_ = head_ws_bytes(max_batch);
  DMLC_HIP_CHECK(hipMalloc(&head_ws_, head_ws_bytes_));
  DMLC_HIP_CHECK(hipMemset(head_ws_, 0, head_ws_bytes_));
  // big-tile conv split-K slabs for the largest batch
  long slabs = 0;
  for (const Op& op : ops_) {
    if (op.type != OpType::Conv) continue;
    const ConvArgs a = conv_geom(op, max_batch);
    const int cfg = opt_.bigtile ? conv_bigtile_pick(a, num_cus_) : -1;
    if (cfg >= 0) slabs = std::max(slabs, conv_bigtile_slabs(a, cfg, conv_bigtile_splits(a, cfg, num_cus_)));
  }
  if (bt_ws_) DMLC_HIP_CHECK(hipFree(bt_ws_));
  bt_ws_bytes_ = conv_bigtile_ws_bytes(slabs);
  DMLC_HIP_CHECK(hipMalloc(&bt_ws_, bt_ws_bytes_));
  DMLC_HIP_CHECK(hipMemset(bt_ws_, 0, conv_bigtile_ws_header_bytes()));
}

double Engine::gflop_per_image() const {
  double f = 0;
  for (const auto& op : ops_) {
    if (op.type != OpType::Conv && op.type != OpType::StemPool) continue;
    const ConvLayer& L = convs_[op.conv];
    ActShape o = shapes_[op.out];
    if (op.type == OpType::StemPool) o.H = o.W = image_size_ / 2;  // the conv's (pre-pool) output
    f += 2.0 * o.H * o.W * L.cout * (double)L.cin * L.kh * L.kw;
  }
  return f * 1e-9;
}

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

void Engine::bind(ConvArgs& a, const Op& op, float* logits) const {
  const ConvLayer& L = convs_[op.conv];
  const uint8_t* wa = (const uint8_t*)warena_;
  a.x = acts_[op.in];
  a.zero = zero_;
  a.w = wa + L.w_off;
  a.bias = (const float*)(wa + L.b_off);
  a.res = op.res >= 0 ? acts_[op.res] : nullptr;
  a.y = (a.out_f32 && logits) ? (void*)logits : acts_[op.out];
  a.alpha = L.fp8 ? (const float*)(wa + L.a_off) : nullptr;
  a.ws = ws_;
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
// launch swallows. Reads the graph, the layout pass's offsets (wf_off,
// cat_off, npad) and num_cus_; no device state.
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
    if (opt.small_conv && k3 && L.wf_off && B <= kSmallConvMaxB &&
        conv_small_supported(is.H, is.W, is.C, L.cout, L.stride) &&
        !(opt.direct13 && conv3x3_13_supported(is.H, is.W, is.C, L.cout)))  // (AlexNet keeps its fused pools)
      return Path::Small;
    // layer2's stride-1 convs: one weight-stationary workgroup per image walking
    // its rows (59-60 us vs 62-66 us for the stream conv at B=256,
    // profiles/r2_rows28.txt)
    if (opt.rows28 && (k3 || k3o8) && L.stride == 1 && L.wf_off && full_rounds() &&
        conv3x3_rows28_supported(is.H, is.W, is.C, L.cout))
      return Path::Rows28;
    if (opt.direct13 && k3 && L.stride == 1 && L.wf_off && conv3x3_13_supported(is.H, is.W, is.C, L.cout))
      return Path::Direct13;
    // e4m3 in and out (fp8_3x3_in): whole images per workgroup, once the batch
    // fills the CUs (query batches: the e4m3 implicit GEMM)
    if (L.fp8 && !L.fc && L.kh == 3 && L.kw == 3 && L.pad == 1 && L.wf_off && op.res < 0 && shapes[op.out].fp8 &&
        4 * B >= cus && conv3x3_stream8_supported(is.H, is.W, is.C, L.cout, L.stride))
      return Path::Stream8;
    if (opt.direct27 && L.plain() && L.kh == 5 && L.kw == 5 && L.stride == 1 && L.relu && L.wf_off &&
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
           (path[oi + 1] == Path::Stream || (path[oi + 1] == Path::Small && D.wf_off));
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
    return L1.relu && L2.relu && L1.wf_off && L2.wf_off && conv3x3_block_supported(is.H, is.W, is.C) &&
           L1.cout == is.C && L2.cout == is.C && !shapes[c1.in].fp8 && !shapes[c2.out].fp8 &&
           path[oi] == Path::Rows && path[oi + 1] == Path::Rows;
  }

  // a layer1 bottleneck's 3x3 (64 -> 64 on 56x56, fragment-order weights), as bottleneck56.hip runs it
  static bool bottleneck_conv2(const ConvLayer& L2) {
    return L2.kh == 3 && L2.kw == 3 && L2.stride == 1 && L2.pad == 1 && L2.relu && L2.cout == 64 && L2.wf_off &&
           L2.kpad == 576;
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
    if (!bottleneck_conv2(convs[c2.conv]) || !e.bottleneck_conv3(L3) || !L3.wf_off || !L3.relu) return false;
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
    return opt.s2rows && op.res < 0 && L.wf_off && D.wf_off && full_rounds() &&
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
    if (!L2.wf_off || !D.wf_off || L2.fp8 || shapes[c2.out].fp8 || path[oi + 1] != Path::Rows28) return false;
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
        if (!D && opt.s2rows128 && op.res < 0 && L.wf_off && L.stride == 2 && full_rounds() &&
            conv3x3_s2rows128_supported(is.H, is.W, is.C, L.cout)) {
          st.kernel = Kernel::S2Rows128;
          break;
        }
        st.kernel = Kernel::Stream;
        st.ds_op = ds;
        // (wf_off may exist for conv3x3_s2rows alone)
        st.wreg = L.wf_off && opt.stream_wreg && (!D || D->wf_off) &&
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
        st.wreg = L.wf_off && opt.rows_wreg;
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
            st.wreg = opt.stem_dense && L.wf_off;
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

int Engine::feature_dim() const {
  for (const Op& op : ops_)
    if (op.type == OpType::Conv && op.out == logits_act_) return convs_[op.conv].cin;
  throw std::logic_error("feature_dim: no fc writes the logits");
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

// ---------------------------------------------------------------- executor
void Engine::run_ops(const std::vector<Step>& steps, const Request& req, hipStream_t s, std::vector<hipEvent_t>* evs,
                     bool trace) {
  const Input& in = req.in;
  const int B = req.B;
  int32_t* const idx = req.idx;
  float *const prob = req.prob, *const logits = req.logits, *const features = req.features;
  // the u8 kernels and PackTensor each read their own kind of input: a plan
  // made for the other kind is refused before anything is launched
  for (const Step& st : steps) {
    const bool u8 = st.kernel == Kernel::AlexStem || st.kernel == Kernel::Preprocess || st.kernel == Kernel::StemPoolU8;
    if ((u8 && in.tensor) || (st.kernel == Kernel::PackTensor && !in.tensor))
      throw std::logic_error(std::string("plan step ") + kernel_name(st.kernel) + " does not read this input");
    if (st.kernel == Kernel::Embed && !features) throw std::logic_error("plan step Embed without a features buffer");
  }
  if (features && (steps.empty() || steps.back().kernel != Kernel::Embed))
    throw std::logic_error("a features buffer needs a plan made with features");
  const uint8_t* const images = in.tensor ? nullptr : (const uint8_t*)in.data;
  size_t ei = 0;
  if (evs) DMLC_HIP_CHECK(hipEventRecord((*evs)[ei++], s));
  std::map<int, hipEvent_t> joined;  // activation -> event its side-stream producer recorded
  const uint8_t* wa = (const uint8_t*)warena_;
  auto W = [&](size_t off) { return (const void*)(wa + off); };
  auto F = [&](size_t off) { return (const float*)(wa + off); };
  // an e4m3 output's epilogue scale (0: bf16 output)
  auto inv_scale = [&](int act) { return shapes_[act].fp8 ? 1.f / shapes_[act].scale : 0.f; };
  // the tail's top-1: the caller's buffers, or scratch when there are none or
  // when they are the [B, k] outputs of a final SoftmaxTopK step
  bool topk = false;
  for (const Step& st : steps) topk |= st.kernel == Kernel::SoftmaxTopK;
  int32_t* const idx_out = (idx && !topk) ? idx : dummy_idx_;
  float* const prob_out = (prob && !topk) ? prob : (float*)(dummy_idx_ + max_batch_);
  for (const Step& st : steps) {
    const size_t oi = st.first_op;
    const Op& op = ops_[oi];
    std::optional<TraceRange> tr;  // per-op host ranges (not inside a graph capture)
    if (trace && st.kernel != Kernel::None) tr.emplace(op.name.c_str());
    hipStream_t cs = s;
    if (st.side) {
      DMLC_HIP_CHECK(hipEventRecord(fork_evs_[oi], s));
      DMLC_HIP_CHECK(hipStreamWaitEvent(side_, fork_evs_[oi], 0));
      cs = side_;
    }
    if (st.kernel != Kernel::None && op.res >= 0 && joined.count(op.res)) {
      DMLC_HIP_CHECK(hipStreamWaitEvent(s, joined[op.res], 0));
      joined.erase(op.res);
    }
    // the step's (first) conv layer, its input shape, and the downsample it computes
    const ConvLayer* Lp = op.conv >= 0 ? &convs_[op.conv] : nullptr;
    const ActShape* isp = op.in >= 0 ? &shapes_[op.in] : nullptr;
    const Op* d = st.ds_op >= 0 ? &ops_[st.ds_op] : nullptr;
    const ConvLayer* D = d ? &convs_[d->conv] : nullptr;
    const void* res = op.res >= 0 ? acts_[op.res] : nullptr;
    void* ypool = st.pool_op >= 0 ? acts_[ops_[st.pool_op].out] : nullptr;
    switch (st.kernel) {
      case Kernel::None:
        break;
      case Kernel::AlexStem: {
        const ConvLayer& L = convs_[ops_[oi + 1].conv];
        alex_stem_u8(images, W(L.wf_off), F(L.b_off), acts_[ops_[oi + 2].out], B, s);
        break;
      }
      case Kernel::Preprocess: {
        const bool paired = op.k == 1;
        const int Wr = paired ? 2 * shapes_[op.out].W : shapes_[op.out].W;
        preprocess_u8(images, acts_[op.out], B, in.Hin, in.Win, image_size_, op.pad, Wr, s, paired);
        break;
      }
      case Kernel::PackTensor: {
        const bool paired = op.k == 1;
        const int Wr = paired ? 2 * shapes_[op.out].W : shapes_[op.out].W;
        pack_tensor(in.data, in.dt, in.channels_last, acts_[op.out], B, image_size_, op.pad, Wr, paired, s);
        break;
      }
      case Kernel::StemPoolU8:
        stem_conv_pool_u8(images, W(Lp->w_off), F(Lp->b_off), acts_[op.out], B, image_size_, st.count, s,
                          st.wreg ? W(Lp->wf_off) : nullptr);
        break;
      case Kernel::StemPool:
        stem_conv_pool(acts_[op.in], W(Lp->w_off), F(Lp->b_off), acts_[op.out], B, image_size_, isp->W, st.count, s);
        break;
      case Kernel::FcSmall: {
        const ConvLayer& L = *Lp;
        const ActShape& os = shapes_[op.out];
        fc_small(acts_[op.in], L.cin, W(L.w_off), L.kpad, F(L.b_off), (os.f32 && logits) ? (void*)logits : acts_[op.out],
                 L.cout, os.f32, B, L.cin, L.cout, L.npad, L.relu, cs);
        break;
      }
      case Kernel::Conv1x1Cat: {
        ConvArgs a = conv_geom(op, B);
        bind(a, op, logits);
        a.split_k = 1;
        a.res = nullptr;
        a.x2 = acts_[d->in];
        a.cin2 = D->cin;
        a.Kpad = Lp->kpad + D->kpad;
        a.w = W(Lp->cat_off);
        a.bias = F(Lp->cat_b_off);
        conv1x1(a, num_cus_, cs);
        break;
      }
      case Kernel::Conv1x1Chain: {
        ConvArgs a = conv_geom(op, B), ra = conv_geom(ops_[oi + 1], B);
        bind(a, op, logits);
        bind(ra, ops_[oi + 1], logits);
        a.split_k = ra.split_k = 1;
        conv1x1_chain(a, ra, num_cus_, cs);
        break;
      }
      case Kernel::Bottleneck56: {
        const ConvLayer& L = *Lp;
        const ConvLayer& L2 = convs_[ops_[oi + 1].conv];
        const ConvLayer& L3 = convs_[ops_[oi + 2].conv];
        const int y = ops_[oi + 2].out;
        bottleneck56(acts_[op.in], W(L.w_off), F(L.a_off), F(L.b_off), W(L2.wf_off), F(L2.b_off), W(L3.wf_off),
                     F(L3.b_off), acts_[y], isp->scale, 1.f / shapes_[y].scale, B, s);
        break;
      }
      case Kernel::Bottleneck56Head: {
        const ConvLayer& L2 = convs_[ops_[oi + 1].conv];
        bottleneck56_head(acts_[op.in], W(Lp->w_off), F(Lp->b_off), W(L2.wf_off), F(L2.b_off), acts_[ops_[oi + 1].out],
                          B, s);
        break;
      }
      case Kernel::Block: {
        const ConvLayer& L2 = convs_[ops_[oi + 1].conv];
        conv3x3_block(acts_[op.in], W(Lp->wf_off), F(Lp->b_off), W(L2.wf_off), F(L2.b_off), acts_[ops_[oi + 1].out],
                      zero_, B, s);
        break;
      }
      case Kernel::S2Rows:  // without ds_op the downsample runs inside conv2 (Rows28)
        conv3x3_s2rows(acts_[op.in], W(Lp->wf_off), F(Lp->b_off), D ? W(D->wf_off) : nullptr,
                       D ? F(D->b_off) : nullptr, acts_[op.out], D ? acts_[d->out] : nullptr, zero_, B, Lp->relu, cs);
        break;
      case Kernel::S2Rows128:
        conv3x3_s2rows128(acts_[op.in], W(Lp->wf_off), F(Lp->b_off), acts_[op.out], B, Lp->relu, inv_scale(op.out), cs);
        break;
      case Kernel::Stream: {
        const ConvLayer& L = *Lp;
        conv3x3_stream(acts_[op.in], W(L.w_off), F(L.b_off), res, acts_[op.out], zero_, B, isp->H, isp->W, isp->C,
                       L.cout, L.stride, L.relu, cs, nullptr, D ? W(D->w_off) : nullptr, D ? F(D->b_off) : nullptr,
                       D ? acts_[d->out] : nullptr, st.wreg ? W(L.wf_off) : nullptr,
                       (st.wreg && D) ? W(D->wf_off) : nullptr, ypool, st.store_y, inv_scale(op.out));
        break;
      }
      case Kernel::Direct13:
        conv3x3_13(acts_[op.in], W(Lp->wf_off), F(Lp->b_off), acts_[op.out], zero_, B, isp->C, Lp->cout, Lp->relu, cs,
                   ypool);
        break;
      case Kernel::Direct27:
        conv5x5_27(acts_[op.in], W(Lp->wf_off), F(Lp->b_off), acts_[op.out], zero_, B, cs, ypool);
        break;
      case Kernel::Small:
        conv_small(acts_[op.in], W(Lp->wf_off), F(Lp->b_off), res, acts_[op.out], B, isp->H, isp->W, isp->C, Lp->cout,
                   Lp->stride, Lp->relu, st.count, cs, D ? W(D->wf_off) : nullptr, D ? F(D->b_off) : nullptr,
                   D ? acts_[d->out] : nullptr);
        break;
      case Kernel::Stream8:
        conv3x3_stream8(acts_[op.in], W(Lp->wf_off), F(Lp->a_off), F(Lp->b_off), acts_[op.out], zero_, B, isp->H,
                        isp->W, isp->C, Lp->cout, Lp->stride, Lp->relu, 1.f / shapes_[op.out].scale, cs);
        break;
      case Kernel::Rows28:
        if (D)  // the block's downsample as 2 more K steps instead of the residual read
          conv3x3_rows28(acts_[op.in], W(Lp->wf_off), F(Lp->b_off), nullptr, acts_[op.out], B, Lp->relu, cs, 0.f,
                         acts_[d->in], W(D->wf_off), F(D->b_off));
        else
          conv3x3_rows28(acts_[op.in], W(Lp->wf_off), F(Lp->b_off), res, acts_[op.out], B, Lp->relu, cs,
                         inv_scale(op.out));
        break;
      case Kernel::Rows:
        conv3x3_rows(acts_[op.in], W(Lp->w_off), F(Lp->b_off), res, acts_[op.out], zero_, B, isp->H, isp->W, isp->C,
                     Lp->relu, st.count, cs, st.wreg ? W(Lp->wf_off) : nullptr);
        break;
      case Kernel::Conv1x1: {
        ConvArgs a = conv_geom(op, B);
        bind(a, op, logits);
        a.split_k = 1;
        conv1x1(a, num_cus_, cs);
        break;
      }
      case Kernel::BigTile: {
        ConvArgs a = conv_geom(op, B);
        bind(a, op, logits);
        // (a slab reserved for a smaller max_batch: no K split)
        const int splits = conv_bigtile_ws_bytes(conv_bigtile_slabs(a, st.cfg, st.count)) > bt_ws_bytes_ ? 1 : st.count;
        conv2d_bigtile(a, st.cfg, splits, bt_ws_, bt_ws_bytes_, cs);
        break;
      }
      case Kernel::Igemm: {
        ConvArgs a = conv_geom(op, B);
        bind(a, op, logits);
        if (st.side) a.split_k = 1;  // the split-K workspace belongs to the main stream
        conv2d_igemm(a, cs);
        break;
      }
      case Kernel::FcGemm: {
        ConvArgs a = conv_geom(op, B);
        bind(a, op, logits);
        fc_gemm(a, st.count, cs);
        break;
      }
      case Kernel::MaxPool: {
        const ActShape& o = shapes_[op.out];
        maxpool2d(acts_[op.in], acts_[op.out], B, isp->H, isp->W, isp->C, o.H, o.W, op.k, op.stride, op.pad, s);
        break;
      }
      case Kernel::AvgPoolGlobal:
        avgpool_global(acts_[op.in], acts_[op.out], B, isp->H * isp->W, isp->C, s, isp->fp8, isp->scale);
        break;
      case Kernel::HeadPooled:  // op = the fc on the pooled rows, then softmax / top-1
        head_pooled(acts_[op.in], W(Lp->w_off), F(Lp->b_off), B, Lp->cin, Lp->cout, Lp->kpad, Lp->npad,
                    logits ? logits : (float*)acts_[op.out], idx_out, prob_out, head_ws_, head_ws_bytes_, num_cus_, s);
        break;
      case Kernel::HeadFused: {  // op = the avgpool, then fc and softmax / top-1
        const ConvLayer& L = convs_[ops_[oi + 1].conv];
        head_fused(acts_[op.in], W(L.w_off), F(L.b_off), B, isp->H * isp->W, isp->C, L.cout, L.kpad, L.npad,
                   logits ? logits : (float*)acts_[ops_[oi + 1].out], idx_out, prob_out, head_ws_, head_ws_bytes_,
                   num_cus_, s, isp->fp8, isp->scale);
        break;
      }
      case Kernel::AvgPoolAdaptive: {
        const ActShape& o = shapes_[op.out];
        avgpool_adaptive(acts_[op.in], acts_[op.out], B, isp->H, isp->W, isp->C, o.H, o.W, s);
        break;
      }
      case Kernel::SoftmaxTop1:
        softmax_top1(logits ? logits : (const float*)acts_[op.in], B, num_classes_, num_classes_, idx_out, prob_out, s);
        break;
      case Kernel::SoftmaxTopK:  // on the logits the tail wrote
        softmax_topk(logits ? logits : (const float*)acts_[logits_act_], B, num_classes_, num_classes_, st.count, idx,
                     prob, s);
        break;
      case Kernel::Embed: {  // the fc's input, or the fused head's pooled as the head pools it
        const int src = ops_[st.src_op].out;
        const ActShape& ss = shapes_[src];
        if (st.count > 0)
          embed_rows(acts_[src], features, B, st.count, ss.C, ss.fp8, ss.scale, req.l2norm, s);
        else
          embed_rows(acts_[src], features, B, 1, (int)ss.elems_per_image(), false, 1.f, req.l2norm, s);
        break;
      }
    }
    if (st.side) {
      DMLC_HIP_CHECK(hipEventRecord(join_evs_[oi], side_));
      joined[op.out] = join_evs_[oi];
    }
    for (int i = 0; evs && i < st.n_ops; ++i) DMLC_HIP_CHECK(hipEventRecord((*evs)[ei++], s));
  }
}

void Engine::forward(const uint8_t* images, int B, int Hin, int Win, int32_t* idx, float* prob,
                     float* logits, hipStream_t stream, bool use_graph) {
  forward(Request{Input{images, Hin, Win}, B, 1, idx, prob, logits}, stream, use_graph);
}

void Engine::forward(const Request& req, hipStream_t stream, bool use_graph) {
  if (req.in.tensor && req.in.dt != TensorDType::F32 && req.in.dt != TensorDType::F16 && req.in.dt != TensorDType::BF16)
    throw std::invalid_argument("forward_tensor: unknown dtype");
  if (req.B <= 0) return;
  check_topk(req.k);
  if (req.k > 1 && (!req.idx || !req.prob)) throw std::invalid_argument("top-k: null idx / prob");
  if (req.B > max_batch_) throw std::invalid_argument("batch exceeds reserved max_batch");
  if (!req.in.data) throw std::invalid_argument("null images");
  DMLC_HIP_CHECK(hipSetDevice(device_));
  // Forwards share the activation arena: one on a different stream than the
  // previous forward is ordered after it (an event, only then).
  if (last_stream_valid_ && stream != last_stream_) DMLC_HIP_CHECK(hipStreamWaitEvent(stream, ev_out_, 0));
  if (use_graph) {
    // Replays go straight onto the caller's stream: no event hop to the
    // engine's stream and back (two cross-stream waits cost ~40 us of idle
    // GPU between back-to-back forwards: profiles/r1_graph_gap.txt). The
    // engine's own stream is only used to capture.
    const GraphKey key = key_of(req);
    auto it = graphs_.find(key);
    if (it == graphs_.end()) {
      const std::vector<Step> steps = plan(spec_for(req, false));
      DMLC_HIP_CHECK(hipStreamSynchronize(stream));
      hipGraph_t g;
      DMLC_HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
      run_ops(steps, req, stream_, nullptr, false);
      DMLC_HIP_CHECK(hipStreamEndCapture(stream_, &g));
      hipGraphExec_t ex;
      DMLC_HIP_CHECK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
      DMLC_HIP_CHECK(hipGraphDestroy(g));
      it = graphs_.emplace(key, ex).first;
    }
    DMLC_TRACE("engine.forward(graph)");
    DMLC_HIP_CHECK(hipGraphLaunch(it->second, stream));
  } else {  // eager launches straight onto the caller's stream
    DMLC_TRACE("engine.forward");
    run_ops(plan(spec_for(req, true)), req, stream, nullptr, true);
  }
  DMLC_HIP_CHECK(hipEventRecord(ev_out_, stream));
  last_stream_ = stream;
  last_stream_valid_ = true;
}

std::vector<std::pair<std::string, float>> Engine::profile(const uint8_t* images, int B, int Hin,
                                                           int Win, hipStream_t stream) {
  if (B > max_batch_) throw std::invalid_argument("batch exceeds reserved max_batch");
  DMLC_HIP_CHECK(hipSetDevice(device_));
  DMLC_HIP_CHECK(hipStreamSynchronize(stream));
  std::vector<hipEvent_t> evs(ops_.size() + 1);
  for (auto& e : evs) DMLC_HIP_CHECK(hipEventCreate(&e));
  // per-op event timing keeps every op on one stream
  const Request req{Input{images, Hin, Win}, B};
  PlanSpec spec = spec_for(req, true);
  spec.side = false;
  run_ops(plan(spec), req, stream_, &evs, true);
  DMLC_HIP_CHECK(hipStreamSynchronize(stream_));
  std::vector<std::pair<std::string, float>> out;
  for (size_t i = 0; i < ops_.size(); ++i) {
    float ms = 0;
    DMLC_HIP_CHECK(hipEventElapsedTime(&ms, evs[i], evs[i + 1]));
    out.emplace_back(ops_[i].name, ms);
  }
  for (auto& e : evs) hipEventDestroy(e);
  return out;
}

}  // namespace dmlc
