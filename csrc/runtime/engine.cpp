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
#include <optional>
#include <stdexcept>

#include "trace.h"

namespace dmlc {

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

int Engine::feature_dim() const {
  for (const Op& op : ops_)
    if (op.type == OpType::Conv && op.out == logits_act_) return convs_[op.conv].cin;
  throw std::logic_error("feature_dim: no fc writes the logits");
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
