// pybind11 module `_C`: the Python face of the native runtime.
//
// Device buffers cross the boundary as raw pointers (ints) plus a raw
// hipStream_t, so this module does not depend on PyTorch's HIP headers; the
// Python wrappers in `dmlc.ops` / `dmlc.runtime` pass `tensor.data_ptr()` and
// `torch.cuda.current_stream().cuda_stream`.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include "../serve/shard.h"
#include <pybind11/stl.h>

#include <map>

#include "../kernels/kernels.h"
#include "../runtime/engine.h"
#include "../runtime/gallery.h"
#include "../runtime/jpeg.h"
#include "../runtime/jpeg_gpu.h"
#include "../runtime/ot_io.h"

namespace py = pybind11;
using namespace dmlc;

namespace {

template <typename T>
T* P(uintptr_t v) {
  return reinterpret_cast<T*>(v);
}
hipStream_t S(uintptr_t v) { return reinterpret_cast<hipStream_t>(v); }

WeightMap to_weight_map(const py::dict& d) {
  WeightMap w;
  for (auto item : d) {
    auto name = py::cast<std::string>(item.first);
    auto arr = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(item.second);
    if (!arr) throw std::invalid_argument("weight " + name + " is not convertible to float32");
    HostTensor h;
    for (py::ssize_t i = 0; i < arr.ndim(); ++i) h.shape.push_back(arr.shape(i));
    h.data.assign(arr.data(), arr.data() + arr.size());
    w.emplace(name, std::move(h));
  }
  return w;
}

py::dict from_weight_map(const WeightMap& w) {
  py::dict d;
  for (const auto& kv : w) {
    std::vector<py::ssize_t> shape(kv.second.shape.begin(), kv.second.shape.end());
    py::array_t<float> a(shape);
    std::copy(kv.second.data.begin(), kv.second.data.end(), a.mutable_data());
    d[py::str(kv.first)] = a;
  }
  return d;
}

// JpegLayout <-> {"width", "height", "ncomp", "hmax", "vmax", "comps": [{"h", "v", "bw", "bh", "offset", "qt"}]}
py::dict layout_to_dict(const JpegLayout& l) {
  py::dict d;
  d["width"] = l.width;
  d["height"] = l.height;
  d["ncomp"] = l.ncomp;
  d["hmax"] = l.hmax;
  d["vmax"] = l.vmax;
  py::list comps;
  for (int i = 0; i < l.ncomp; ++i) {
    py::dict c;
    c["h"] = l.comp[i].h;
    c["v"] = l.comp[i].v;
    c["bw"] = l.comp[i].bw;
    c["bh"] = l.comp[i].bh;
    c["offset"] = l.comp[i].offset;
    py::array_t<uint16_t> q(64);
    std::copy(l.comp[i].qt, l.comp[i].qt + 64, q.mutable_data());
    c["qt"] = q;
    comps.append(c);
  }
  d["comps"] = comps;
  return d;
}

JpegLayout layout_from_dict(const py::dict& d) {
  JpegLayout l;
  l.width = py::cast<int>(d["width"]);
  l.height = py::cast<int>(d["height"]);
  l.hmax = py::cast<int>(d["hmax"]);
  l.vmax = py::cast<int>(d["vmax"]);
  const py::list comps = d["comps"];
  if (comps.size() < 1 || comps.size() > 3) throw std::invalid_argument("jpeg layout: 1 to 3 components");
  l.ncomp = (int)comps.size();
  if (d.contains("ncomp") && py::cast<int>(d["ncomp"]) != l.ncomp) throw std::invalid_argument("jpeg layout: ncomp");
  size_t off = 0;
  for (int i = 0; i < l.ncomp; ++i) {
    const py::dict c = comps[i];
    JpegComp& lc = l.comp[i];
    lc.h = py::cast<int>(c["h"]);
    lc.v = py::cast<int>(c["v"]);
    lc.bw = c.contains("bw") ? py::cast<int>(c["bw"]) : 0;
    lc.bh = c.contains("bh") ? py::cast<int>(c["bh"]) : 0;
    if (lc.bw < 0 || lc.bh < 0 || lc.bw > 4096 || lc.bh > 4096) throw std::invalid_argument("jpeg layout: block counts");
    lc.offset = c.contains("offset") ? py::cast<size_t>(c["offset"]) : off;
    off = lc.offset + (size_t)lc.bw * lc.bh * 64;
    if (c.contains("qt")) {
      auto q = py::array_t<uint16_t, py::array::c_style | py::array::forcecast>::ensure(c["qt"]);
      if (!q || q.size() != 64) throw std::invalid_argument("jpeg layout: qt must hold 64 values");
      std::copy(q.data(), q.data() + 64, lc.qt);
    }
  }
  return l;
}

// a host copy of device descriptors, as jpeg_gpu_plan returned it
// compute units of the current device
int device_cus() {
  hipDeviceProp_t prop;
  int dev = 0;
  DMLC_HIP_CHECK(hipGetDevice(&dev));
  DMLC_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  return prop.multiProcessorCount;
}

// a 1x1 / stride-1 conv's ConvArgs for the conv1x1_chain bindings (e4m3 in and out, ReLU)
ConvArgs chain_conv(uintptr_t x, uintptr_t w, uintptr_t alpha, uintptr_t bias, uintptr_t res, uintptr_t y, int B, int H,
                    int W, int Cin, int N, float res_scale, float out_inv_scale, bool relu, uintptr_t zero) {
  ConvArgs a;
  a.x = P<void>(x);
  a.w = P<void>(w);
  a.alpha = P<float>(alpha);
  a.bias = P<float>(bias);
  a.res = P<void>(res);
  a.y = P<void>(y);
  a.zero = P<void>(zero);
  a.B = B;
  a.H = a.Ho = H;
  a.W = a.Wo = W;
  a.Cin = a.Kpad = Cin;
  a.N = a.Npad = a.ldo = N;
  a.relu = relu;
  a.in_fp8 = a.out_fp8 = true;
  a.res_scale = res_scale;
  a.out_inv_scale = out_inv_scale;
  return a;
}

const JpegGpuImage* host_descs(const py::array_t<uint8_t, py::array::c_style>& a, int* n) {
  if (a.size() % (py::ssize_t)sizeof(JpegGpuImage)) throw std::invalid_argument("jpeg descriptors: bad size");
  *n = (int)(a.size() / (py::ssize_t)sizeof(JpegGpuImage));
  return reinterpret_cast<const JpegGpuImage*>(a.data());
}

}  // namespace

void bind_dp(py::module& m);  // py_dp.cpp

// {"fused_block": false, ...} -> EngineOptions (unknown names are errors)
static EngineOptions engine_options(const std::map<std::string, bool>& m) {
  EngineOptions o;
  for (const auto& kv : m)
    if (!o.set(kv.first, kv.second)) throw std::invalid_argument("unknown engine option: " + kv.first);
  return o;
}

PYBIND11_MODULE(_C, m) {
  m.doc() = "dmlc native runtime: CDNA4 HIP kernels, inference engine, .ot I/O";

  // ---------------------------------------------------------------- ops
  m.def("conv_kpad", &conv_kpad, py::arg("Cin"), py::arg("KH"), py::arg("KW"), py::arg("stem") = false);
  m.def("stem_row_width", &stem_row_width);
  m.def("conv_npad", &conv_npad);
  m.def("conv_out_dim", &conv_out_dim);
  m.def(
      "conv2d",
      [](uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t res, uintptr_t y, int B, int H, int W,
         int Cin, int KH, int KW, int stride, int pad, int N, int Npad, int Kpad, int ldo, bool relu,
         bool out_f32, int split_k, uintptr_t ws, int tile, uintptr_t zero, bool stem, int Ho, int Wo,
         int max_blocks, uintptr_t stream, bool in_fp8, bool out_fp8, uintptr_t alpha, float res_scale,
         float out_inv_scale, uintptr_t bt_ws, size_t bt_ws_bytes, int bt_splits, int num_cus, uintptr_t x2,
         int cin2) {
        if ((x2 || cin2) && tile != kConv1x1Tile)
          throw std::invalid_argument("conv2d: x2 / cin2 (a second input along K) need the CONV_1X1 route");
        ConvArgs a;
        a.x2 = P<void>(x2);
        a.cin2 = cin2;
        a.x = P<void>(x);
        a.zero = P<void>(zero);
        a.stem = stem;
        a.w = P<void>(w);
        a.bias = P<float>(bias);
        a.res = P<void>(res);
        a.y = P<void>(y);
        a.B = B;
        a.H = H;
        a.W = W;
        a.Cin = Cin;
        a.KH = KH;
        a.KW = KW;
        a.stride = stride;
        a.pad = pad;
        a.Ho = Ho > 0 ? Ho : conv_out_dim(H, KH, stride, pad);
        a.Wo = Wo > 0 ? Wo : conv_out_dim(W, KW, stride, pad);
        a.N = N;
        a.Npad = Npad;
        a.Kpad = Kpad;
        a.ldo = ldo;
        a.relu = relu;
        a.out_f32 = out_f32;
        a.split_k = split_k;
        a.ws = P<float>(ws);
        a.tile = tile;
        a.persistent = max_blocks > 0;
        a.max_blocks = max_blocks;
        a.in_fp8 = in_fp8;
        a.out_fp8 = out_fp8;
        a.alpha = P<float>(alpha);
        a.res_scale = res_scale;
        a.out_inv_scale = out_inv_scale;
        if (tile == kConv1x1Tile) {  // weight-stationary 1x1 conv (conv1x1.hip)
          a.tile = -1;
          conv1x1(a, num_cus > 0 ? num_cus : device_cus(), S(stream));  // num_cus sizes the persistent grid
          return;
        }
        if (tile == kConv1x1Tile + 2) {  // fully connected (fc_gemm.hip); split_k 0: fc_gemm_splits
          a.tile = -1;
          hipDeviceProp_t prop;
          int dev = 0;
          DMLC_HIP_CHECK(hipGetDevice(&dev));
          DMLC_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
          fc_gemm(a, split_k > 0 ? split_k : fc_gemm_splits(a, prop.multiProcessorCount), S(stream));
          return;
        }
        if (tile == kConv1x1Tile + 1) {  // support query only (no launch): raises if unsupported
          a.tile = -1;
          if (!conv1x1_supported(a)) throw std::invalid_argument("conv1x1: unsupported shape");
          return;
        }
        if (tile == kConvBigTile0 + 2) {  // persistent 256x128 big tiles
          a.tile = -1;
          hipDeviceProp_t prop;
          int dev = 0;
          DMLC_HIP_CHECK(hipGetDevice(&dev));
          DMLC_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
          conv2d_bigtile_persistent(a, max_blocks > 0 ? max_blocks : conv_bigtile_persistent_grid(a, prop.multiProcessorCount),
                                    S(stream));
          return;
        }
        if (tile >= kConvBigTile0) {  // 8-wave big-tile configs (conv_bigtile.hip)
          a.tile = -1;
          conv2d_bigtile(a, tile - kConvBigTile0, bt_splits, P<void>(bt_ws), bt_ws_bytes, S(stream));
          return;
        }
        conv2d_igemm(a, S(stream));
      },
      py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("res"), py::arg("y"), py::arg("B"),
      py::arg("H"), py::arg("W"), py::arg("Cin"), py::arg("KH"), py::arg("KW"), py::arg("stride"),
      py::arg("pad"), py::arg("N"), py::arg("Npad"), py::arg("Kpad"), py::arg("ldo"),
      py::arg("relu"), py::arg("out_f32"), py::arg("split_k"), py::arg("ws"), py::arg("tile"),
      py::arg("zero"), py::arg("stem"), py::arg("Ho"), py::arg("Wo"), py::arg("max_blocks"),
      py::arg("stream"), py::arg("in_fp8") = false, py::arg("out_fp8") = false, py::arg("alpha") = 0,
      py::arg("res_scale") = 1.f, py::arg("out_inv_scale") = 1.f, py::arg("bt_ws") = 0, py::arg("bt_ws_bytes") = 0,
      py::arg("bt_splits") = 1, py::arg("num_cus") = 0, py::arg("x2") = 0, py::arg("cin2") = 0);
  m.def("conv_bigtile_ws_bytes", &conv_bigtile_ws_bytes);
  m.def("conv_bigtile_ws_header_bytes", &conv_bigtile_ws_header_bytes);
  m.def(
      "conv_bigtile_splits",
      [](int B, int Ho, int Wo, int Npad, int Kpad, int cfg, int num_cus) {
        ConvArgs a;
        a.B = B;
        a.Ho = Ho;
        a.Wo = Wo;
        a.Npad = Npad;
        a.Kpad = Kpad;
        return conv_bigtile_splits(a, cfg, num_cus);
      });
  m.attr("CONV_BIGTILE0") = kConvBigTile0;
  m.attr("CONV_1X1") = kConv1x1Tile;
  m.attr("CONV_FC") = kConv1x1Tile + 2;
  m.def("fc_gemm_splits", [](int M, int Kpad, int Npad, int num_cus) {
    ConvArgs a;
    a.B = M;
    a.Kpad = Kpad;
    a.Npad = Npad;
    return fc_gemm_splits(a, num_cus);
  });
  m.def("maxpool2d", [](uintptr_t x, uintptr_t y, int B, int H, int W, int C, int k, int stride,
                        int pad, uintptr_t stream) {
    maxpool2d(P<void>(x), P<void>(y), B, H, W, C, conv_out_dim(H, k, stride, pad),
              conv_out_dim(W, k, stride, pad), k, stride, pad, S(stream));
  });
  m.def("avgpool_global", [](uintptr_t x, uintptr_t y, int B, int HW, int C, uintptr_t stream) {
    avgpool_global(P<void>(x), P<void>(y), B, HW, C, S(stream));
  });
  m.def("avgpool_adaptive", [](uintptr_t x, uintptr_t y, int B, int H, int W, int C, int Ho, int Wo,
                               uintptr_t stream) {
    avgpool_adaptive(P<void>(x), P<void>(y), B, H, W, C, Ho, Wo, S(stream));
  });
  m.def(
      "preprocess_u8",
      [](uintptr_t x, uintptr_t y, int B, int Hin, int Win, int S_, int pad, int Wr, uintptr_t stream,
         bool paired) { preprocess_u8(P<uint8_t>(x), P<void>(y), B, Hin, Win, S_, pad, Wr, S(stream), paired); },
      py::arg("x"), py::arg("y"), py::arg("B"), py::arg("Hin"), py::arg("Win"), py::arg("S"), py::arg("pad"),
      py::arg("Wr"), py::arg("stream"), py::arg("paired") = false);
  py::enum_<TensorDType>(m, "TensorDType")
      .value("F32", TensorDType::F32)
      .value("F16", TensorDType::F16)
      .value("BF16", TensorDType::BF16);
  m.def(
      "pack_tensor",
      [](uintptr_t x, TensorDType dt, bool channels_last, uintptr_t y, int B, int S_, int pad, int Wr, bool paired,
         uintptr_t stream) { pack_tensor(P<void>(x), dt, channels_last, P<void>(y), B, S_, pad, Wr, paired, S(stream)); },
      py::arg("x"), py::arg("dtype"), py::arg("channels_last"), py::arg("y"), py::arg("B"), py::arg("S"),
      py::arg("pad"), py::arg("Wr"), py::arg("paired"), py::arg("stream"));
  m.attr("STEM_POOL_K") = kStemPoolK;
  m.def("stem_pool_pick_strip", &stem_pool_pick_strip);
  m.def("stem_pool_u8_pick_strip", &stem_pool_u8_pick_strip);
  m.def("conv3x3_stream_supported", &conv3x3_stream_supported, py::arg("Hin"), py::arg("Win"), py::arg("Cin"),
        py::arg("Cout"), py::arg("stride") = 1);
  m.def("conv3x3_stream", [](uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t res, uintptr_t y, uintptr_t zero,
                             int B, int H, int W, int Cin, int Cout, int stride, bool relu, uintptr_t stream,
                             uintptr_t stamps, uintptr_t wd, uintptr_t bd, uintptr_t yd, uintptr_t wfrag,
                             uintptr_t wdfrag, uintptr_t pool, bool store_y, float out_inv_scale) {
    conv3x3_stream(P<void>(x), P<void>(w), P<float>(bias), P<void>(res), P<void>(y), P<void>(zero), B, H, W, Cin, Cout,
                   stride, relu, S(stream), P<unsigned long long>(stamps), P<void>(wd), P<float>(bd), P<void>(yd),
                   P<void>(wfrag), P<void>(wdfrag), P<void>(pool), store_y, out_inv_scale);
  }, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("res"), py::arg("y"), py::arg("zero"), py::arg("B"),
        py::arg("H"), py::arg("W"), py::arg("Cin"), py::arg("Cout"), py::arg("stride"), py::arg("relu"),
        py::arg("stream"), py::arg("stamps") = 0, py::arg("wd") = 0, py::arg("bd") = 0, py::arg("yd") = 0,
        py::arg("wfrag") = 0, py::arg("wdfrag") = 0, py::arg("pool") = 0, py::arg("store_y") = true,
        py::arg("out_inv_scale") = 0.f);
  m.def("conv3x3_stream_pool_supported", &conv3x3_stream_pool_supported);
  m.def("conv3x3_stream_uses_frag", &conv3x3_stream_uses_frag);
  m.def("conv3x3_stream_set_variant", &conv3x3_stream_set_variant);
  m.def("conv3x3_rows_supported", &conv3x3_rows_supported);
  m.def("conv3x3_rows_pick_strip", &conv3x3_rows_pick_strip);
  m.def("conv3x3_rows", [](uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t res, uintptr_t y, uintptr_t zero,
                           int B, int H, int W, int C, bool relu, int strip, uintptr_t stream, uintptr_t wfrag) {
    conv3x3_rows(P<void>(x), P<void>(w), P<float>(bias), P<void>(res), P<void>(y), P<void>(zero), B, H, W, C, relu,
                 strip, S(stream), P<void>(wfrag));
  }, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("res"), py::arg("y"), py::arg("zero"), py::arg("B"),
        py::arg("H"), py::arg("W"), py::arg("C"), py::arg("relu"), py::arg("strip"), py::arg("stream"),
        py::arg("wfrag") = 0);
  m.def("conv3x3_block_supported", &conv3x3_block_supported);
  m.def("conv3x3_block", [](uintptr_t x, uintptr_t wf1, uintptr_t b1, uintptr_t wf2, uintptr_t b2, uintptr_t y,
                            uintptr_t zero, int B, uintptr_t stream) {
    conv3x3_block(P<void>(x), P<void>(wf1), P<float>(b1), P<void>(wf2), P<float>(b2), P<void>(y), P<void>(zero), B,
                  S(stream));
  }, py::arg("x"), py::arg("wf1"), py::arg("b1"), py::arg("wf2"), py::arg("b2"), py::arg("y"), py::arg("zero"),
        py::arg("B"), py::arg("stream"));
  m.def("bottleneck56", [](uintptr_t x, uintptr_t w1, uintptr_t a1, uintptr_t b1, uintptr_t wf2, uintptr_t b2,
                           uintptr_t wf3, uintptr_t b3, uintptr_t y, float res_scale, float out_inv_scale, int B,
                           uintptr_t stream) {
    bottleneck56(P<void>(x), P<void>(w1), P<float>(a1), P<float>(b1), P<void>(wf2), P<float>(b2), P<void>(wf3),
                 P<float>(b3), P<void>(y), res_scale, out_inv_scale, B, S(stream));
  }, py::arg("x"), py::arg("w1"), py::arg("a1"), py::arg("b1"), py::arg("wf2"), py::arg("b2"), py::arg("wf3"),
     py::arg("b3"), py::arg("y"), py::arg("res_scale"), py::arg("out_inv_scale"), py::arg("B"), py::arg("stream") = 0);
  m.def("bottleneck56_supported", &bottleneck56_supported, py::arg("H"), py::arg("W"), py::arg("C"), py::arg("Cm"));
  m.def("bottleneck56_head", [](uintptr_t x, uintptr_t w1, uintptr_t b1, uintptr_t wf2, uintptr_t b2, uintptr_t y, int B,
                                uintptr_t stream) {
    bottleneck56_head(P<void>(x), P<void>(w1), P<float>(b1), P<void>(wf2), P<float>(b2), P<void>(y), B, S(stream));
  }, py::arg("x"), py::arg("w1"), py::arg("b1"), py::arg("wf2"), py::arg("b2"), py::arg("y"), py::arg("B"),
     py::arg("stream") = 0);
  // conv1x1_chain: the expand conv (x [B,H,W,Cin] e4m3 -> y [B,H,W,N] e4m3, + res) and the reduce conv on y
  // (-> y2 [B,H,W,N2] e4m3); the *_supported form takes the same arguments and launches nothing
  auto chain_args = [](uintptr_t x, uintptr_t w, uintptr_t alpha, uintptr_t bias, uintptr_t res, uintptr_t y,
                       uintptr_t w2, uintptr_t alpha2, uintptr_t bias2, uintptr_t y2, int B, int H, int W, int Cin,
                       int N, int N2, float res_scale, float out_inv_scale, float out_inv_scale2, bool relu, bool relu2,
                       uintptr_t zero) {
    return std::make_pair(
        chain_conv(x, w, alpha, bias, res, y, B, H, W, Cin, N, res_scale, out_inv_scale, relu, zero),
        chain_conv(y, w2, alpha2, bias2, 0, y2, B, H, W, N, N2, 1.f, out_inv_scale2, relu2, zero));
  };
  m.def("conv1x1_chain_supported", [=](uintptr_t x, uintptr_t w, uintptr_t alpha, uintptr_t bias, uintptr_t res,
                                       uintptr_t y, uintptr_t w2, uintptr_t alpha2, uintptr_t bias2, uintptr_t y2, int B,
                                       int H, int W, int Cin, int N, int N2, float res_scale, float out_inv_scale,
                                       float out_inv_scale2, bool relu, bool relu2, uintptr_t zero) {
    const auto ar = chain_args(x, w, alpha, bias, res, y, w2, alpha2, bias2, y2, B, H, W, Cin, N, N2, res_scale,
                               out_inv_scale, out_inv_scale2, relu, relu2, zero);
    return conv1x1_chain_supported(ar.first, ar.second);
  }, py::arg("x"), py::arg("w"), py::arg("alpha"), py::arg("bias"), py::arg("res"), py::arg("y"), py::arg("w2"),
     py::arg("alpha2"), py::arg("bias2"), py::arg("y2"), py::arg("B"), py::arg("H"), py::arg("W"), py::arg("Cin"),
     py::arg("N"), py::arg("N2"), py::arg("res_scale") = 1.f, py::arg("out_inv_scale") = 1.f,
     py::arg("out_inv_scale2") = 1.f, py::arg("relu") = true, py::arg("relu2") = true, py::arg("zero") = 0);
  m.def("conv1x1_chain", [=](uintptr_t x, uintptr_t w, uintptr_t alpha, uintptr_t bias, uintptr_t res, uintptr_t y,
                             uintptr_t w2, uintptr_t alpha2, uintptr_t bias2, uintptr_t y2, int B, int H, int W, int Cin,
                             int N, int N2, float res_scale, float out_inv_scale, float out_inv_scale2, bool relu,
                             bool relu2, uintptr_t zero, int num_cus, uintptr_t stream) {
    const auto ar = chain_args(x, w, alpha, bias, res, y, w2, alpha2, bias2, y2, B, H, W, Cin, N, N2, res_scale,
                               out_inv_scale, out_inv_scale2, relu, relu2, zero);
    conv1x1_chain(ar.first, ar.second, num_cus > 0 ? num_cus : device_cus(), S(stream));
  }, py::arg("x"), py::arg("w"), py::arg("alpha"), py::arg("bias"), py::arg("res"), py::arg("y"), py::arg("w2"),
     py::arg("alpha2"), py::arg("bias2"), py::arg("y2"), py::arg("B"), py::arg("H"), py::arg("W"), py::arg("Cin"),
     py::arg("N"), py::arg("N2"), py::arg("res_scale"), py::arg("out_inv_scale"), py::arg("out_inv_scale2"),
     py::arg("relu"), py::arg("relu2"), py::arg("zero"), py::arg("num_cus") = 0, py::arg("stream") = 0);
  // AlexNet's shape-specialised kernels
  m.attr("ALEX_STEM_K") = kAlexStemK;
  m.def("alex_stem_k", &alex_stem_k);
  m.def("alex_stem_supported", &alex_stem_supported);
  m.def("alex_stem_u8", [](uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t y, int B, uintptr_t stream) {
    alex_stem_u8(P<uint8_t>(x), P<void>(w), P<float>(bias), P<void>(y), B, S(stream));
  }, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"), py::arg("B"), py::arg("stream"));
  m.def("conv5x5_27_supported", &conv5x5_27_supported);
  m.def("conv5x5_27", [](uintptr_t x, uintptr_t wf, uintptr_t bias, uintptr_t y, uintptr_t zero, int B,
                         uintptr_t stream, uintptr_t ypool) {
    conv5x5_27(P<void>(x), P<void>(wf), P<float>(bias), P<void>(y), P<void>(zero), B, S(stream), P<void>(ypool));
  }, py::arg("x"), py::arg("wf"), py::arg("bias"), py::arg("y"), py::arg("zero"), py::arg("B"), py::arg("stream"),
        py::arg("ypool") = 0);
  m.def("conv3x3_13_supported", &conv3x3_13_supported);
  m.def("conv3x3_13_pool_supported", &conv3x3_13_pool_supported);
  m.def("conv3x3_13", [](uintptr_t x, uintptr_t wf, uintptr_t bias, uintptr_t y, uintptr_t zero, int B, int Cin,
                         int Cout, bool relu, uintptr_t stream, uintptr_t ypool) {
    conv3x3_13(P<void>(x), P<void>(wf), P<float>(bias), P<void>(y), P<void>(zero), B, Cin, Cout, relu, S(stream),
               P<void>(ypool));
  }, py::arg("x"), py::arg("wf"), py::arg("bias"), py::arg("y"), py::arg("zero"), py::arg("B"), py::arg("Cin"),
        py::arg("Cout"), py::arg("relu"), py::arg("stream"), py::arg("ypool") = 0);
  m.def("fc_small_supported", &fc_small_supported);
  m.def("fc_small", [](uintptr_t x, int ldx, uintptr_t w, int ldw, uintptr_t bias, uintptr_t y, int ldo, bool out_f32,
                       int B, int K, int N, int Npad, bool relu, uintptr_t stream) {
    fc_small(P<void>(x), ldx, P<void>(w), ldw, P<float>(bias), P<void>(y), ldo, out_f32, B, K, N, Npad, relu,
             S(stream));
  }, py::arg("x"), py::arg("ldx"), py::arg("w"), py::arg("ldw"), py::arg("bias"), py::arg("y"), py::arg("ldo"),
        py::arg("out_f32"), py::arg("B"), py::arg("K"), py::arg("N"), py::arg("Npad"), py::arg("relu"),
        py::arg("stream"));
  m.def("conv3x3_stream8_supported", &conv3x3_stream8_supported);
  m.def("conv3x3_stream8_frag_offset", &conv3x3_stream8_frag_offset);
  m.def("conv3x3_stream8_set_variant", &conv3x3_stream8_set_variant);
  m.def("conv3x3_stream8", [](uintptr_t x, uintptr_t wf, uintptr_t alpha, uintptr_t bias, uintptr_t y, uintptr_t zero,
                              int B, int H, int W, int Cin, int Cout, int stride, bool relu, float out_inv_scale,
                              uintptr_t stream) {
    conv3x3_stream8(P<void>(x), P<void>(wf), P<float>(alpha), P<float>(bias), P<void>(y), P<void>(zero), B, H, W, Cin,
                    Cout, stride, relu, out_inv_scale, S(stream));
  }, py::arg("x"), py::arg("wf"), py::arg("alpha"), py::arg("bias"), py::arg("y"), py::arg("zero"), py::arg("B"),
        py::arg("H"), py::arg("W"), py::arg("Cin"), py::arg("Cout"), py::arg("stride"), py::arg("relu"),
        py::arg("out_inv_scale"), py::arg("stream") = 0);
  m.def("conv3x3_s2rows_supported", &conv3x3_s2rows_supported);
  m.def("conv3x3_s2rows128_supported", &conv3x3_s2rows128_supported);
  m.def("conv3x3_s2rows128", [](uintptr_t x, uintptr_t wf, uintptr_t bias, uintptr_t y, int B, bool relu,
                                float out_inv_scale, uintptr_t stream) {
    conv3x3_s2rows128(P<void>(x), P<void>(wf), P<float>(bias), P<void>(y), B, relu, out_inv_scale, S(stream));
  }, py::arg("x"), py::arg("wf"), py::arg("bias"), py::arg("y"), py::arg("B"), py::arg("relu"),
        py::arg("out_inv_scale"), py::arg("stream"));
  m.def("conv3x3_s2rows", [](uintptr_t x, uintptr_t wf, uintptr_t bias, uintptr_t wdf, uintptr_t bd, uintptr_t y,
                             uintptr_t yd, uintptr_t zero, int B, bool relu, uintptr_t stream) {
    conv3x3_s2rows(P<void>(x), P<void>(wf), P<float>(bias), P<void>(wdf), P<float>(bd), P<void>(y), P<void>(yd),
                   P<void>(zero), B, relu, S(stream));
  }, py::arg("x"), py::arg("wf"), py::arg("bias"), py::arg("wdf"), py::arg("bd"), py::arg("y"), py::arg("yd"),
        py::arg("zero"), py::arg("B"), py::arg("relu"), py::arg("stream"));
  m.def("conv_small_supported", &conv_small_supported);
  m.def("conv_small_pick_mf", &conv_small_pick_mf);
  m.def("conv_small_set_mf", &conv_small_set_mf);
  m.def("conv_small", [](uintptr_t x, uintptr_t wf, uintptr_t bias, uintptr_t res, uintptr_t y, int B, int H, int W,
                         int CI, int CO, int stride, bool relu, int mf, uintptr_t stream, uintptr_t wdf, uintptr_t bd,
                         uintptr_t yd) {
    conv_small(P<void>(x), P<void>(wf), P<float>(bias), P<void>(res), P<void>(y), B, H, W, CI, CO, stride, relu, mf,
               S(stream), P<void>(wdf), P<float>(bd), P<void>(yd));
  }, py::arg("x"), py::arg("wf"), py::arg("bias"), py::arg("res"), py::arg("y"), py::arg("B"), py::arg("H"),
        py::arg("W"), py::arg("CI"), py::arg("CO"), py::arg("stride"), py::arg("relu"), py::arg("mf"),
        py::arg("stream"), py::arg("wdf") = 0, py::arg("bd") = 0, py::arg("yd") = 0);
  m.def("conv3x3_rows28_supported", &conv3x3_rows28_supported);
  m.def("conv3x3_rows28", [](uintptr_t x, uintptr_t wf, uintptr_t bias, uintptr_t res, uintptr_t y, int B, bool relu,
                             uintptr_t stream, float out_inv_scale, uintptr_t xds, uintptr_t wds, uintptr_t bds) {
    conv3x3_rows28(P<void>(x), P<void>(wf), P<float>(bias), P<void>(res), P<void>(y), B, relu, S(stream),
                   out_inv_scale, P<void>(xds), P<void>(wds), P<float>(bds));
  }, py::arg("x"), py::arg("wf"), py::arg("bias"), py::arg("res"), py::arg("y"), py::arg("B"), py::arg("relu"),
        py::arg("stream"), py::arg("out_inv_scale") = 0.f, py::arg("xds") = 0, py::arg("wds") = 0,
        py::arg("bds") = 0);
  m.def("stem_conv_pool_u8", [](uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t y, int B, int S_, int strip,
                                uintptr_t stream, uintptr_t w_dense) {
    stem_conv_pool_u8(P<uint8_t>(x), P<void>(w), P<float>(bias), P<void>(y), B, S_, strip, S(stream),
                      P<void>(w_dense));
  }, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"), py::arg("B"), py::arg("S"), py::arg("strip"),
        py::arg("stream"), py::arg("w_dense") = 0);
  m.def("stem_dense_k_index", &stem_dense_k_index);
  m.def("stem_conv_pool_set_dbg", &stem_conv_pool_set_dbg);
  m.def("stem_conv_pool_set_stamps", [](uintptr_t p) { stem_conv_pool_set_stamps((void*)p); });
  // StaggerKernel families (kernels.h), for kernel_stagger / kernel_stagger_set
  m.attr("STAG_STREAM") = (int)kStagStream;
  m.attr("STAG_ROWS28") = (int)kStagRows28;
  m.def("kernel_stagger", &kernel_stagger);
  m.def("kernel_stagger_set", &kernel_stagger_set);
  m.def("kernel_stagger_for_lanes", &kernel_stagger_for_lanes);
  m.def("stem_conv_pool", [](uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t y, int B, int S_, int Wq,
                             int strip, uintptr_t stream) {
    stem_conv_pool(P<void>(x), P<void>(w), P<float>(bias), P<void>(y), B, S_, Wq, strip, S(stream));
  });
  m.def("mfma_fp8_probe", [](uintptr_t a, uintptr_t b, uintptr_t d, uintptr_t stream) {
    mfma_fp8_probe(P<void>(a), P<void>(b), P<float>(d), S(stream));
  });
  m.def("head_ws_bytes", &head_ws_bytes);
  m.def("head_pooled_splits", &head_pooled_splits);
  m.def("head_splits", &head_splits);
  m.def("head_supported", &head_supported);
  m.def("head_fused", [](uintptr_t x, uintptr_t w, uintptr_t bias, int B, int HW, int C, int N, int ldw, int Npad,
                         uintptr_t logits, uintptr_t idx, uintptr_t prob, uintptr_t ws, size_t ws_bytes, int num_cus,
                         uintptr_t stream, bool in_fp8, float scale) {
    head_fused(P<void>(x), P<void>(w), P<float>(bias), B, HW, C, N, ldw, Npad, P<float>(logits), P<int32_t>(idx),
               P<float>(prob), P<void>(ws), ws_bytes, num_cus, S(stream), in_fp8, scale);
  }, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("B"), py::arg("HW"), py::arg("C"), py::arg("N"),
        py::arg("ldw"), py::arg("Npad"), py::arg("logits"), py::arg("idx"), py::arg("prob"), py::arg("ws"),
        py::arg("ws_bytes"), py::arg("num_cus"), py::arg("stream"), py::arg("in_fp8") = false, py::arg("scale") = 1.f);
  m.def("conv1x1_plan", [](bool in8, bool out8, int rb, int nw, bool res, int s, int wv, bool ch) {
    const C1Plan p = conv1x1_plan(in8, out8, rb, nw, res, s, wv, ch);
    py::dict d;
    d["s"] = p.s;
    d["dt"] = p.dt;
    d["rt"] = p.rt;
    d["st"] = p.st;
    d["st2"] = p.st2;
    d["pre"] = p.pre;
    d["n1"] = p.n1;
    d["n1_first"] = p.n1_first;
    d["pro_wait"] = p.pro_wait;
    d["pro_wait_ch"] = p.pro_wait_ch;
    d["res_wait"] = p.res_wait;
    return d;
  });
  m.def("head_pooled", [](uintptr_t pooled, uintptr_t w, uintptr_t bias, int B, int C, int N, int ldw, int Npad,
                          uintptr_t logits, uintptr_t idx, uintptr_t prob, uintptr_t ws, size_t ws_bytes, int num_cus,
                          uintptr_t stream, int ns, int ko) {
    head_pooled(P<void>(pooled), P<void>(w), P<float>(bias), B, C, N, ldw, Npad, P<float>(logits), P<int32_t>(idx),
                P<float>(prob), P<void>(ws), ws_bytes, num_cus, S(stream), ns, ko);
  }, py::arg("pooled"), py::arg("w"), py::arg("bias"), py::arg("B"), py::arg("C"), py::arg("N"), py::arg("ldw"),
        py::arg("Npad"), py::arg("logits"), py::arg("idx"), py::arg("prob"), py::arg("ws"), py::arg("ws_bytes"),
        py::arg("num_cus"), py::arg("stream"), py::arg("ns") = 0, py::arg("ko") = 0);
  m.def("softmax_top1", [](uintptr_t logits, int B, int N, int ld, uintptr_t idx, uintptr_t prob,
                           uintptr_t stream) {
    softmax_top1(P<float>(logits), B, N, ld, P<int32_t>(idx), P<float>(prob), S(stream));
  });
  m.attr("MAX_TOPK") = kMaxTopK;
  m.def("softmax_topk", [](uintptr_t logits, int B, int N, int ld, int k, uintptr_t idx, uintptr_t prob,
                           uintptr_t stream) {
    softmax_topk(P<float>(logits), B, N, ld, k, P<int32_t>(idx), P<float>(prob), S(stream));
  }, py::arg("logits"), py::arg("B"), py::arg("N"), py::arg("ld"), py::arg("k"), py::arg("idx"), py::arg("prob"),
        py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("embed_rows_supported", &embed_rows_supported, py::arg("HW"), py::arg("C"));
  m.def("embed_rows", [](uintptr_t x, uintptr_t out, int B, int HW, int C, bool in_fp8, float scale, bool l2norm,
                         uintptr_t stream) {
    embed_rows(P<void>(x), P<float>(out), B, HW, C, in_fp8, scale, l2norm, S(stream));
  }, py::arg("x"), py::arg("out"), py::arg("B"), py::arg("HW"), py::arg("C"), py::arg("in_fp8"), py::arg("scale"),
        py::arg("l2norm"), py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  // nearest-neighbour search (sim_topk.hip); the sizing functions need no device
  m.def("sim_topk_supported", &sim_topk_supported, py::arg("D"));
  m.def("sim_topk_slices", &sim_topk_slices, py::arg("B"), py::arg("N"), py::arg("num_cus"));
  m.def("sim_topk_max_slices", &sim_topk_max_slices, py::arg("N"));
  m.def("sim_topk_slice_rows", [](long N, int slices, int slice) {
    long first = 0, end = 0;
    sim_topk_slice_rows(N, slices, slice, &first, &end);
    return py::make_tuple(first, end);
  }, py::arg("N"), py::arg("slices"), py::arg("slice"));
  m.def("sim_topk_ws_bytes", &sim_topk_ws_bytes, py::arg("B"), py::arg("k"), py::arg("slices"));
  m.def("sim_topk", [](uintptr_t q, TensorDType qdt, uintptr_t q_scale, uintptr_t g, uintptr_t g_scale, int B, long N,
                       int D, int k, uintptr_t idx, uintptr_t score, uintptr_t ws, size_t ws_bytes, int num_cus,
                       uintptr_t stream, int slices, uintptr_t g_label, uintptr_t q_want) {
    sim_topk(P<void>(q), qdt, P<float>(q_scale), P<void>(g), P<float>(g_scale), B, N, D, k, P<int32_t>(idx),
             P<float>(score), P<void>(ws), ws_bytes, num_cus, S(stream), slices, P<int32_t>(g_label),
             P<int32_t>(q_want));
  }, py::arg("q"), py::arg("dtype"), py::arg("q_scale"), py::arg("g"), py::arg("g_scale"), py::arg("B"), py::arg("N"),
        py::arg("D"), py::arg("k"), py::arg("idx"), py::arg("score"), py::arg("ws"), py::arg("ws_bytes"),
        py::arg("num_cus"), py::arg("stream"), py::arg("slices") = 0, py::arg("g_label") = 0, py::arg("q_want") = 0,
        py::call_guard<py::gil_scoped_release>());
  m.def("knn_vote", [](uintptr_t idx, uintptr_t score, uintptr_t g_label, long N, int B, int k, bool weighted,
                       uintptr_t label, uintptr_t share, uintptr_t stream) {
    knn_vote(P<int32_t>(idx), P<float>(score), P<int32_t>(g_label), N, B, k, weighted, P<int32_t>(label),
             P<float>(share), S(stream));
  }, py::arg("idx"), py::arg("score"), py::arg("g_label"), py::arg("N"), py::arg("B"), py::arg("k"),
        py::arg("weighted"), py::arg("label"), py::arg("share"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("gallery_pack", [](uintptr_t rows, uintptr_t g, uintptr_t inv_norm, int M, int D, uintptr_t stream) {
    gallery_pack(P<float>(rows), P<void>(g), P<float>(inv_norm), M, D, S(stream));
  }, py::arg("rows"), py::arg("g"), py::arg("inv_norm"), py::arg("M"), py::arg("D"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  // the e4m3 gallery (sim_topk.hip): quantiser and search
  m.def("sim_topk8_supported", &sim_topk8_supported, py::arg("D"));
  m.def("sim_topk8_ws_bytes", &sim_topk8_ws_bytes, py::arg("B"), py::arg("k"), py::arg("slices"));
  m.def("gallery_pack8", [](uintptr_t rows, TensorDType dt, uintptr_t codes, uintptr_t scale, bool cosine, int M, int D,
                            uintptr_t stream) {
    gallery_pack8(P<void>(rows), dt, P<void>(codes), P<float>(scale), cosine, M, D, S(stream));
  }, py::arg("rows"), py::arg("dtype"), py::arg("codes"), py::arg("scale"), py::arg("cosine"), py::arg("M"),
        py::arg("D"), py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("sim_topk8", [](uintptr_t q, TensorDType qdt, uintptr_t g_codes, uintptr_t g_scale, bool cosine, int B, long N,
                        int D, int k, uintptr_t idx, uintptr_t score, uintptr_t ws, size_t ws_bytes, int num_cus,
                        uintptr_t stream, int slices, uintptr_t g_label, uintptr_t q_want) {
    sim_topk8(P<void>(q), qdt, P<void>(g_codes), P<float>(g_scale), cosine, B, N, D, k, P<int32_t>(idx),
              P<float>(score), P<void>(ws), ws_bytes, num_cus, S(stream), slices, P<int32_t>(g_label),
              P<int32_t>(q_want));
  }, py::arg("q"), py::arg("dtype"), py::arg("g_codes"), py::arg("g_scale"), py::arg("cosine"), py::arg("B"),
        py::arg("N"), py::arg("D"), py::arg("k"), py::arg("idx"), py::arg("score"), py::arg("ws"), py::arg("ws_bytes"),
        py::arg("num_cus"), py::arg("stream"), py::arg("slices") = 0, py::arg("g_label") = 0, py::arg("q_want") = 0,
        py::call_guard<py::gil_scoped_release>());
  py::class_<Gallery>(m, "Gallery")
      .def(py::init([](int dim, long capacity, int device, const std::string& metric, int max_batch,
                       const std::string& dtype) {
             if (metric != "cosine" && metric != "dot")
               throw std::invalid_argument("Gallery: metric is \"cosine\" or \"dot\", got " + metric);
             if (dtype != "bf16" && dtype != "e4m3")
               throw std::invalid_argument("Gallery: dtype is \"bf16\" or \"e4m3\", got " + dtype);
             return new Gallery(dim, capacity, device, metric == "cosine", max_batch,
                                dtype == "e4m3" ? GalleryDType::E4M3 : GalleryDType::BF16);
           }),
           py::arg("dim"), py::arg("capacity"), py::arg("device") = 0, py::arg("metric") = "cosine",
           py::arg("max_batch") = 256, py::arg("dtype") = "bf16")
      .def_property_readonly("dtype",
                             [](const Gallery& g) {
                               return std::string(g.dtype() == GalleryDType::E4M3 ? "e4m3" : "bf16");
                             })
      .def_property_readonly("dim", &Gallery::dim)
      .def_property_readonly("capacity", &Gallery::capacity)
      .def_property_readonly("device", &Gallery::device)
      .def_property_readonly("max_batch", &Gallery::max_batch)
      .def_property_readonly("size", &Gallery::size)
      .def_property_readonly("metric", [](const Gallery& g) { return std::string(g.cosine() ? "cosine" : "dot"); })
      .def_property_readonly("live", &Gallery::live)
      .def("add",
           [](Gallery& g, uintptr_t rows, int M, uintptr_t stream, uintptr_t labels) {
             return g.add(P<float>(rows), M, P<int32_t>(labels), S(stream));
           },
           py::arg("rows"), py::arg("M"), py::arg("stream"), py::arg("labels") = 0,
           py::call_guard<py::gil_scoped_release>())
      .def("remove",
           [](Gallery& g, const std::vector<long>& ids, uintptr_t stream) {
             g.remove(ids.data(), (long)ids.size(), S(stream));
           },
           py::arg("ids"), py::arg("stream"), py::call_guard<py::gil_scoped_release>())
      .def("search",
           [](Gallery& g, uintptr_t q, TensorDType qdt, int B, int k, uintptr_t idx, uintptr_t score, uintptr_t stream,
              uintptr_t q_want) {
             g.search(P<void>(q), qdt, B, k, P<int32_t>(idx), P<float>(score), S(stream), P<int32_t>(q_want));
           },
           py::arg("q"), py::arg("dtype"), py::arg("B"), py::arg("k"), py::arg("idx"), py::arg("score"),
           py::arg("stream"), py::arg("q_want") = 0, py::call_guard<py::gil_scoped_release>())
      .def("classify",
           [](Gallery& g, uintptr_t q, TensorDType qdt, int B, int k, bool weighted, uintptr_t label, uintptr_t share,
              uintptr_t stream) {
             g.classify(P<void>(q), qdt, B, k, weighted, P<int32_t>(label), P<float>(share), S(stream));
           },
           py::arg("q"), py::arg("dtype"), py::arg("B"), py::arg("k"), py::arg("weighted"), py::arg("label"),
           py::arg("share"), py::arg("stream"), py::call_guard<py::gil_scoped_release>())
      .def("read_labels",
           [](Gallery& g, uintptr_t dst, uintptr_t stream) { g.read_labels(P<int32_t>(dst), S(stream)); },
           py::arg("dst"), py::arg("stream"), py::call_guard<py::gil_scoped_release>())
      .def("clear", &Gallery::clear);

  // ---------------------------------------------------------------- jpeg
  m.def("decode_jpeg", [](py::bytes data) {
    std::string s = data;
    Image img;
    {
      py::gil_scoped_release nogil;
      img = decode_jpeg((const uint8_t*)s.data(), s.size());
    }
    py::array_t<uint8_t> a({img.height, img.width, 3});
    std::copy(img.rgb.begin(), img.rgb.end(), a.mutable_data());
    return a;
  });
  // ragged resize: descs = packed ImageDesc records (device memory), out u8 [B, S, S, 3]
  m.attr("IMAGE_DESC_BYTES") = (int)sizeof(ImageDesc);
  m.def("resize_u8_ragged", [](uintptr_t descs, uintptr_t out, int B, int S_, uintptr_t stream, bool antialias) {
    resize_u8_ragged(P<ImageDesc>(descs), P<uint8_t>(out), B, S_, S(stream), antialias);
  }, py::arg("descs"), py::arg("out"), py::arg("B"), py::arg("S"), py::arg("stream"), py::arg("antialias") = false);
  // its host reference: u8 [H, W, 3] -> u8 [S, S, 3]
  m.def("resize_u8_host", [](const py::array_t<uint8_t, py::array::c_style | py::array::forcecast>& rgb, int S_,
                             bool antialias) {
    if (rgb.ndim() != 3 || rgb.shape(2) != 3) throw std::invalid_argument("resize_u8_host: expected u8 [H, W, 3]");
    Image img;
    img.height = (int)rgb.shape(0);
    img.width = (int)rgb.shape(1);
    img.rgb.assign(rgb.data(), rgb.data() + rgb.size());
    std::vector<uint8_t> r;
    {
      py::gil_scoped_release nogil;
      r = resize_u8_host(img, S_, antialias);
    }
    py::array_t<uint8_t> a({S_, S_, 3});
    std::copy(r.begin(), r.end(), a.mutable_data());
    return a;
  }, py::arg("rgb"), py::arg("size"), py::arg("antialias") = false);
  // split decode: entropy decoding on the host -> (layout, int16 coefficients)
  m.def("decode_jpeg_coeffs", [](py::bytes data) {
    std::string s = data;
    std::vector<int16_t> buf;
    JpegLayout l;
    {
      py::gil_scoped_release nogil;
      l = decode_jpeg_coeffs((const uint8_t*)s.data(), s.size(), [&](size_t n) {
        buf.resize(n);
        return buf.data();
      });
    }
    py::array_t<int16_t> a((py::ssize_t)buf.size());
    std::copy(buf.begin(), buf.end(), a.mutable_data());
    return py::make_tuple(layout_to_dict(l), a);
  });
  m.def("jpeg_gpu_supported", [](const py::dict& layout) { return jpeg_gpu_supported(layout_from_dict(layout)); });
  // the decoder's colour stage on caller-supplied planes (u8 [8 bh][8 bw] each) -> [height][width][3]
  m.def("ycc_planes_to_rgb", [](const std::vector<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>& planes,
                                const py::dict& layout) {
    const JpegLayout l = layout_from_dict(layout);
    if (!jpeg_gpu_supported(l)) throw std::invalid_argument("ycc_planes_to_rgb: unsupported layout");
    if ((int)planes.size() != l.ncomp) throw std::invalid_argument("ycc_planes_to_rgb: one plane per component");
    const uint8_t* ptr[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < l.ncomp; ++i) {
      const JpegComp& c = l.comp[i];
      const int cw = (l.width * c.h + l.hmax - 1) / l.hmax, ch = (l.height * c.v + l.vmax - 1) / l.vmax;
      if (planes[i].ndim() != 2 || planes[i].shape(0) != 8 * c.bh || planes[i].shape(1) != 8 * c.bw)
        throw std::invalid_argument("ycc_planes_to_rgb: plane " + std::to_string(i) + " is not [8 bh][8 bw]");
      if (cw > 8 * c.bw || ch > 8 * c.bh) throw std::invalid_argument("ycc_planes_to_rgb: plane smaller than the image");
      ptr[i] = planes[i].data();
    }
    py::array_t<uint8_t> out({l.height, l.width, 3});
    ycc_planes_to_rgb(ptr, l, out.mutable_data());
    return out;
  });
  // device descriptors for a batch whose coefficients and planes lie back to
  // back in image order: (descriptors as bytes, tables float32 [T][64],
  // coefficient count, plane bytes)
  m.def("jpeg_gpu_plan", [](const std::vector<py::dict>& layouts, const std::vector<uintptr_t>& rgb) {
    if (layouts.size() != rgb.size()) throw std::invalid_argument("jpeg_gpu_plan: one destination per image");
    py::array_t<uint8_t> descs((py::ssize_t)(layouts.size() * sizeof(JpegGpuImage)));
    auto* d = reinterpret_cast<JpegGpuImage*>(descs.mutable_data());
    std::vector<float> tables;
    size_t coef = 0, plane = 0;
    for (size_t i = 0; i < layouts.size(); ++i) {
      JpegLayout l = layout_from_dict(layouts[i]);
      size_t off = 0;  // components back to back, whatever the dict's offsets say
      for (int c = 0; c < l.ncomp; ++c) {
        l.comp[c].offset = off;
        off += (size_t)l.comp[c].bw * l.comp[c].bh * 64;
      }
      const int t0 = (int)(tables.size() / 64);
      d[i] = jpeg_gpu_image(l, P<uint8_t>(rgb[i]), coef, plane, t0);
      tables.resize(tables.size() + 64 * (size_t)l.ncomp);
      jpeg_gpu_tables(l, tables.data() + 64 * (size_t)t0);
      coef += l.total();
      plane += jpeg_plane_bytes(l);
    }
    py::array_t<float> t({(py::ssize_t)(tables.size() / 64), (py::ssize_t)64});
    std::copy(tables.begin(), tables.end(), t.mutable_data());
    return py::make_tuple(descs, t, coef, plane);
  });
  m.def("jpeg_idct_planes", [](const py::array_t<uint8_t, py::array::c_style>& descs, uintptr_t dev, uintptr_t qf,
                               int n_tables, uintptr_t coef, size_t coef_elems, uintptr_t planes, size_t plane_bytes,
                               uintptr_t stream) {
    int n = 0;
    const JpegGpuImage* h = host_descs(descs, &n);
    jpeg_idct_planes(h, P<JpegGpuImage>(dev), n, P<float>(qf), n_tables, P<int16_t>(coef), coef_elems,
                     P<uint8_t>(planes), plane_bytes, S(stream));
  }, py::arg("descs"), py::arg("dev"), py::arg("qf"), py::arg("n_tables"), py::arg("coef"), py::arg("coef_elems"),
        py::arg("planes"), py::arg("plane_bytes"), py::arg("stream"));
  m.def("jpeg_planes_to_rgb", [](const py::array_t<uint8_t, py::array::c_style>& descs, uintptr_t dev, uintptr_t planes,
                                 size_t plane_bytes, uintptr_t stream) {
    int n = 0;
    const JpegGpuImage* h = host_descs(descs, &n);
    jpeg_planes_to_rgb(h, P<JpegGpuImage>(dev), n, P<uint8_t>(planes), plane_bytes, S(stream));
  }, py::arg("descs"), py::arg("dev"), py::arg("planes"), py::arg("plane_bytes"), py::arg("stream"));

  // ---------------------------------------------------------------- .ot
  m.def("ot_load", [](const std::string& path) { return from_weight_map(ot_load(path)); });
  m.def("ot_save", [](const std::string& path, const py::dict& d) { ot_save(path, to_weight_map(d)); });
  // where a staged shard replica's images live (csrc/serve/shard.h)
  m.def("shard_slices", [](int64_t n, const std::vector<int>& devices) {
    py::list out;
    for (const auto& s : shard_slices(n, devices)) out.append(py::make_tuple(s.device, s.first, s.n));
    return out;
  });
  m.def("shard_placement", [](int64_t n, const std::vector<std::vector<int>>& parts) {
    py::list out;
    for (const auto& p : shard_placement(n, parts))
      out.append(py::make_tuple(p.copy, p.slice.device, p.slice.first, p.slice.n));
    return out;
  });

  // ---------------------------------------------------------------- engine
  // host-only packing audit: [(layer, kind, off, bytes)], arena bytes
  m.def("pack_audit", [](const std::string& arch, const py::dict& weights, const std::map<std::string, bool>& options,
                         int num_classes, int image_size) {
    size_t total = 0;
    const auto regs = Engine::pack_audit(arch, to_weight_map(weights), engine_options(options), &total,
                                         num_classes, image_size);
    py::list out;
    for (const auto& r : regs) out.append(py::make_tuple(r.layer, r.kind, r.off, r.bytes));
    return py::make_tuple(out, total);
  }, py::arg("arch"), py::arg("weights"), py::arg("options") = std::map<std::string, bool>{},
     py::arg("num_classes") = 1000, py::arg("image_size") = 224);
  // ... and digests of what it packed: arena bytes, FNV-1a of the arena, {kind: digest}, [(layer, kind, off, bytes,
  // digest)], [(layer, FragOrder name)]
  m.def("pack_digest", [](const std::string& arch, const py::dict& weights, const std::map<std::string, bool>& options,
                          int num_classes, int image_size) {
    const PackDigest d = Engine::pack_digest(arch, to_weight_map(weights), engine_options(options), num_classes,
                                             image_size);
    py::list regions;
    for (size_t i = 0; i < d.regions.size(); ++i) {
      const PackRegion& r = d.regions[i];
      regions.append(py::make_tuple(r.layer, r.kind, r.off, r.bytes, d.region_digests[i]));
    }
    return py::make_tuple(d.total, d.arena, d.kinds, regions, d.orders);
  }, py::arg("arch"), py::arg("weights"), py::arg("options") = std::map<std::string, bool>{},
     py::arg("num_classes") = 1000, py::arg("image_size") = 224);
  // host-only launch plan of a graph-captured forward: [(kernel, first op, n_ops, detail)], and the graph's ops
  // in Engine.op_list's format
  auto plan_list = [](const std::vector<Engine::PlanLine>& lines) {
    py::list out;
    for (const auto& l : lines) out.append(py::make_tuple(l.kernel, l.first_op, l.n_ops, l.detail));
    return out;
  };
  auto op_list = [](const std::vector<Op>& ops) {
    py::list l;
    for (const auto& op : ops) l.append(py::make_tuple(op.name, op.in, op.out, op.res));
    return l;
  };
  m.def("plan_audit", [=](const std::string& arch, const py::dict& weights, const std::map<std::string, bool>& options,
                          int B, bool native, int num_cus, int num_classes, int image_size, int topk,
                          bool tensor_in, bool features) {
    std::vector<Op> ops;
    const EngineOptions opt = engine_options(options);
    PlanSpec spec;
    spec.B = B, spec.native = native, spec.side = opt.fork_ds;
    spec.topk = topk, spec.tensor_in = tensor_in, spec.features = features;
    const auto lines = Engine::plan_audit(arch, to_weight_map(weights), opt, spec, num_cus, &ops, num_classes, image_size);
    return py::make_tuple(plan_list(lines), op_list(ops));
  }, py::arg("arch"), py::arg("weights"), py::arg("options") = std::map<std::string, bool>{}, py::arg("B") = 256,
     py::arg("native") = true, py::arg("num_cus") = 256, py::arg("num_classes") = 1000, py::arg("image_size") = 224,
     py::arg("topk") = 1, py::arg("tensor_in") = false, py::arg("features") = false);
  auto request = [](uintptr_t data, int B, int Hin, int Win, int k, uintptr_t idx, uintptr_t prob, uintptr_t logits,
                    uintptr_t features, bool l2norm, bool tensor = false, TensorDType dt = TensorDType::F32,
                    bool channels_last = false) {
    return Engine::Request{Engine::Input{P<void>(data), Hin, Win, tensor, dt, channels_last}, B, k, P<int32_t>(idx),
                           P<float>(prob), P<float>(logits), P<float>(features), l2norm};
  };
  // what tells one captured graph from another (Engine::key_of), as ints; no engine, no device
  m.def("graph_key", [=](uintptr_t images, int B, int Hin, int Win, int k, uintptr_t idx, uintptr_t prob,
                         uintptr_t logits, uintptr_t features, bool l2norm,
                         const std::optional<std::pair<TensorDType, bool>>& tensor) {
    const Engine::GraphKey key = Engine::key_of(
        tensor ? request(images, B, Hin, Win, k, idx, prob, logits, features, l2norm, true, tensor->first, tensor->second)
               : request(images, B, Hin, Win, k, idx, prob, logits, features, l2norm));
    auto U = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    return py::make_tuple(U(key.data), key.B, key.Hin, key.Win, U(key.idx), U(key.prob), U(key.logits), key.k,
                          key.input_kind, U(key.features), (int)key.l2norm);
  }, py::arg("images"), py::arg("B"), py::arg("Hin"), py::arg("Win"), py::arg("k"), py::arg("idx"), py::arg("prob"),
     py::arg("logits"), py::arg("features") = (uintptr_t)0, py::arg("l2norm") = false, py::arg("tensor") = py::none());
  py::class_<Engine>(m, "Engine")
      .def(py::init([](const std::string& arch, const py::dict& weights, int device, int num_classes,
                       int image_size, const std::map<std::string, bool>& options) {
             return new Engine(arch, to_weight_map(weights), device, num_classes, image_size, engine_options(options));
           }),
           py::arg("arch"), py::arg("weights"), py::arg("device") = 0, py::arg("num_classes") = 1000,
           py::arg("image_size") = 224, py::arg("options") = std::map<std::string, bool>{})
      .def_static(
          "from_ot",
          [](const std::string& arch, const std::string& path, int device, int num_classes, int image_size,
             const std::map<std::string, bool>& options) {
            return new Engine(arch, ot_load(path), device, num_classes, image_size, engine_options(options));
          },
          py::arg("arch"), py::arg("path"), py::arg("device") = 0, py::arg("num_classes") = 1000,
          py::arg("image_size") = 224, py::arg("options") = std::map<std::string, bool>{})
      .def("reserve", &Engine::reserve, py::call_guard<py::gil_scoped_release>())
      .def(
          "forward",
          [=](Engine& e, uintptr_t images, int B, int Hin, int Win, uintptr_t idx, uintptr_t prob,
              uintptr_t logits, uintptr_t stream, bool use_graph) {
            e.forward(request(images, B, Hin, Win, 1, idx, prob, logits, 0, false), S(stream), use_graph);
          },
          py::arg("images"), py::arg("B"), py::arg("Hin"), py::arg("Win"), py::arg("idx"),
          py::arg("prob"), py::arg("logits"), py::arg("stream"), py::arg("use_graph") = true,
          py::call_guard<py::gil_scoped_release>())
      .def(
          "forward_topk",
          [=](Engine& e, uintptr_t images, int B, int Hin, int Win, int k, uintptr_t idx, uintptr_t prob,
              uintptr_t logits, uintptr_t stream, bool use_graph, uintptr_t features, bool l2norm) {
            e.forward(request(images, B, Hin, Win, k, idx, prob, logits, features, l2norm), S(stream), use_graph);
          },
          py::arg("images"), py::arg("B"), py::arg("Hin"), py::arg("Win"), py::arg("k"), py::arg("idx"),
          py::arg("prob"), py::arg("logits"), py::arg("stream"), py::arg("use_graph") = true,
          py::arg("features") = (uintptr_t)0, py::arg("l2norm") = false,
          py::call_guard<py::gil_scoped_release>())
      .def(
          "forward_tensor",
          [=](Engine& e, uintptr_t x, TensorDType dt, bool channels_last, int B, int k, uintptr_t idx, uintptr_t prob,
              uintptr_t logits, uintptr_t stream, bool use_graph, uintptr_t features, bool l2norm) {
            e.forward(request(x, B, e.image_size(), e.image_size(), k, idx, prob, logits, features, l2norm, true, dt,
                              channels_last), S(stream), use_graph);
          },
          py::arg("x"), py::arg("dtype"), py::arg("channels_last"), py::arg("B"), py::arg("k"), py::arg("idx"),
          py::arg("prob"), py::arg("logits"), py::arg("stream"), py::arg("use_graph") = true,
          py::arg("features") = (uintptr_t)0, py::arg("l2norm") = false,
          py::call_guard<py::gil_scoped_release>())
      .def("profile",
           [](Engine& e, uintptr_t images, int B, int Hin, int Win, uintptr_t stream) {
             return e.profile(P<uint8_t>(images), B, Hin, Win, S(stream));
           })
      .def("activation_ptr", [](const Engine& e, int id) { return reinterpret_cast<uintptr_t>(e.activation(id)); })
      .def("activation_shape",
           [](const Engine& e, int id) {
             auto s = e.activation_shape(id);
             return py::make_tuple(s.H, s.W, s.C, s.f32);
           })
      .def("op_list", [=](const Engine& e) { return op_list(e.ops()); })
      // the first B images of a stored activation, copied to dst (device, B * H * W * C elements) on `stream`
      .def("read_activation",
           [](const Engine& e, int id, int B, uintptr_t dst, uintptr_t stream) {
             const ActShape s = e.activation_shape(id);
             if (B < 0 || B > e.max_batch()) throw std::invalid_argument("read_activation: B outside 0..max_batch");
             DMLC_HIP_CHECK(hipMemcpyAsync(P<void>(dst), e.activation(id), (size_t)B * s.elems_per_image() * s.elem_bytes(),
                                           hipMemcpyDeviceToDevice, S(stream)));
           })
      // (e4m3, per-tensor scale) of a stored activation
      .def("activation_quant",
           [](const Engine& e, int id) {
             auto s = e.activation_shape(id);
             return py::make_tuple(s.fp8, s.scale);
           })
      .def("plan", [=](const Engine& e, int B, int Hin, int Win, int topk, bool tensor_in, bool features) {
        // planning reads no buffer: any non-null features pointer asks for the Embed step
        const PlanSpec spec = e.spec_for(request(0, B, Hin, Win, topk, 0, 0, 0, features ? 1 : 0, false, tensor_in), false);
        return plan_list(e.plan_lines(e.plan(spec)));
      }, py::arg("B"), py::arg("Hin"), py::arg("Win"), py::arg("topk") = 1, py::arg("tensor_in") = false,
         py::arg("features") = false)
      .def_property_readonly("feature_dim", &Engine::feature_dim)
      .def_property_readonly("num_cus", &Engine::num_cus)
      .def_property_readonly("num_activations", &Engine::num_activations)
      .def_property_readonly("arch", &Engine::arch)
      .def_property_readonly("device", &Engine::device)
      .def_property_readonly("num_classes", &Engine::num_classes)
      .def_property_readonly("image_size", &Engine::image_size)
      .def_property_readonly("max_batch", &Engine::max_batch)
      .def_property_readonly("weight_bytes", &Engine::weight_bytes)
      .def_property_readonly("activation_bytes", &Engine::activation_bytes)
      .def_property_readonly("gflop_per_image", &Engine::gflop_per_image);

  // ---------------------------------------------------------------- data parallel
  bind_dp(m);
}
