// The engine's weight arena (see engine.h): which layer gets which regions
// (layout_weights), what is written into them (pack_host), and the host-only
// audits of both (pack_audit, pack_digest).
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace dmlc {

namespace {

const HostTensor& need(const WeightMap& w, const std::string& k) {
  auto it = w.find(k);
  if (it == w.end()) throw std::runtime_error("missing weight: " + k);
  return it->second;
}

const HostTensor* maybe(const WeightMap& w, const std::string& k) {
  auto it = w.find(k);
  return it == w.end() ? nullptr : &it->second;
}

}  // namespace

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

const char* frag_order_name(FragOrder o) {
  static const char* const names[] = {"None", "Stream", "Stream8", "StemDense", "AlexStem"};
  static_assert(sizeof(names) / sizeof(names[0]) == (size_t)FragOrder::AlexStem + 1, "one name per FragOrder");
  return names[(size_t)o];
}

namespace {

// The kernels' perm32 (csrc/kernels/common.h) on the host: row n = 16nf + r of
// a wave's 32-row weight tile holds channel 8(r>>2) + 4nf + (r&3) of the group.
int perm32_host(int n) {
  const int nf = n >> 4, r = n & 15;
  return 8 * (r >> 2) + 4 * nf + (r & 3);
}

// The size of a layer's fragment-order region.
size_t frag_bytes(const ConvLayer& L) {
  switch (L.frag) {
    case FragOrder::None: return 0;
    case FragOrder::Stream: return (size_t)L.cout * L.kpad * 2;
    case FragOrder::Stream8: return (size_t)L.cout * L.kpad;
    case FragOrder::StemDense: return (size_t)L.cout * kStemDenseK * 2;
    case FragOrder::AlexStem: return (size_t)L.cout * kAlexStemK * 2;
  }
  throw std::logic_error("frag_bytes: unknown order");
}

// Every element of a conv weight [cout][cin][kh][kw] as the bf16 the arena
// holds, the layer's per-output-channel scale folded in: put(n, kh, kw, c, v).
template <class Put>
void for_each_conv_weight(const ConvLayer& L, const HostTensor& W, const std::vector<float>& scale, Put put) {
  for (int n = 0; n < L.cout; ++n)
    for (int c = 0; c < L.cin; ++c)
      for (int i = 0; i < L.kh; ++i)
        for (int j = 0; j < L.kw; ++j)
          put(n, i, j, c, f2bf_host(W.data[(((size_t)n * L.cin + c) * L.kh + i) * L.kw + j] * scale[n]));
}

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

// Which layer gets a second copy of its weights at wf_off, and in which
// kernel's order. The only place that decides it: the layout pass sizes the
// region from the answer, the packer writes that order, and the planner asks
// for the order its kernel reads. The classes below exclude each other (plain()
// is bf16 on an NHWC activation, so no e4m3 and no stem layer; the kernel
// sizes differ); a layer that two of them claimed is refused instead of one
// region being leaked and the later order winning. Reads npad / kpad / fp8,
// which the layout pass sets first.
FragOrder Engine::frag_order(const ConvLayer& L) const {
  const ActShape is = L.in_act >= 0 ? shapes_[L.in_act] : ActShape{};
  FragOrder order = FragOrder::None;
  int claims = 0;
  auto claim = [&](bool yes, FragOrder o) {
    if (!yes) return;
    order = o;
    ++claims;
  };
  // Who gets a bf16 fragment-order copy: the plain 3x3/p1 convs and 1x1/s2
  // downsamples that a kernel reading its weights in that order can run.
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
  claim(small || ((stream || rows) && L.kpad % 32 == 0), FragOrder::Stream);
  // fragment-order copy for conv_direct.hip
  claim(L.plain() && L.kh == 5 && L.kw == 5 && L.stride == 1 && conv5x5_27_supported(is.H, is.W, is.C, L.cout, L.pad),
        FragOrder::Stream);
  // e4m3 fragment-order copy for conv3x3_stream8.hip
  claim(L.fp8 && !L.fc && L.in_act >= 0 && L.kh == 3 && L.kw == 3 && L.pad == 1 && L.kpad == 9 * L.cin &&
            conv3x3_stream8_supported(is.H, is.W, is.C, L.cout, L.stride),
        FragOrder::Stream8);
  claim(bottleneck_conv3(L), FragOrder::Stream);  // fragment-order copy for bottleneck56.hip's expand conv
  // dense-K order for the one-image-per-workgroup stem (stem_dense_k_index)
  claim(L.stem_pool, FragOrder::StemDense);
  claim(L.alex_stem, FragOrder::AlexStem);  // paired-chunk K order for alex_stem.hip
  if (claims > 1) throw std::logic_error("frag_order: more than one kernel's weight order claims " + L.name);
  return order;
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
    L.frag = frag_order(L);
    L.wf_off = 0;
    if (L.frag != FragOrder::None) {
      L.wf_off = off;
      off = align_up(off + frag_bytes(L), 256);
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
    const RegionRef rf = L.frag != FragOrder::None ? region(L, "wf", L.wf_off, frag_bytes(L)) : RegionRef{};
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
      for_each_conv_weight(L, W, scale, [&](int n, int i, int j, int c, uint16_t v) {
        size_t k;
        if (L.stem_pool)  // paired stem: chunk (kw/2) of row kh, slot 3*(kw%2) + c
          k = (size_t)i * 32 + (j / 2) * 8 + (j % 2) * 3 + c;
        else if (L.pair)  // stem: k = kh*CPK*8 + kw*3 + c
          k = (size_t)i * ((L.kw * 3 + 7) / 8) * 8 + j * 3 + c;
        else
          k = (size_t)(i * L.kw + j) * L.cin_eff + c;
        pw((size_t)n * L.kpad + k) = v;
      });
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
    }
    switch (L.frag) {  // the second copy, from the rows written above
      case FragOrder::None:
        break;
      case FragOrder::Stream:  // bf16 fragment order
        for (int n = 0; n < L.cout; ++n)
          for (int k = 0; k < L.kpad; ++k)
            rf.at<uint16_t>(stream_frag_index(n, k, L.kpad)) = pw((size_t)n * L.kpad + k);
        break;
      case FragOrder::Stream8: {  // conv3x3_stream8's fragment order of the e4m3 weights
        const int KT = L.kpad / 128;
        for (int j = 0; j < L.cout / 32; ++j)
          for (int t = 0; t < KT; ++t)
            for (int nf = 0; nf < 2; ++nf)
              for (int h = 0; h < 2; ++h)
                for (int ln = 0; ln < 64; ++ln) {
                  const int fq = ln >> 4, n = 32 * j + perm32_host(16 * nf + (ln & 15));
                  const int k0 = 128 * t + 32 * fq + 16 * (h ^ (fq & 1));
                  rf.copy(conv3x3_stream8_frag_offset(j, t, nf, h, ln, KT), rw.base + (size_t)n * L.kpad + k0, 16);
                }
        break;
      }
      case FragOrder::StemDense:
        for_each_conv_weight(L, W, scale, [&](int n, int i, int j, int c, uint16_t v) {
          rf.at<uint16_t>((size_t)n * kStemDenseK + stem_dense_k_index(i, j, c)) = v;
        });
        break;
      case FragOrder::AlexStem:
        for_each_conv_weight(L, W, scale, [&](int n, int i, int j, int c, uint16_t v) {
          rf.at<uint16_t>((size_t)n * kAlexStemK + alex_stem_k(i, j, c)) = v;
        });
        break;
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

std::vector<PackRegion> Engine::pack_audit(const std::string& arch, const WeightMap& weights,
                                           const EngineOptions& options, size_t* total, int num_classes,
                                           int image_size) {
  Engine e(HostOnly{}, arch, weights, num_classes, image_size, options);
  std::vector<PackRegion> regions;
  const std::vector<uint8_t> host = e.pack_host(weights, &regions);
  if (total) *total = host.size();
  return regions;
}

namespace {
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;
uint64_t fnv1a(const uint8_t* p, size_t n, uint64_t h = kFnvBasis) {
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}
}  // namespace

PackDigest Engine::pack_digest(const std::string& arch, const WeightMap& weights, const EngineOptions& options,
                               int num_classes, int image_size) {
  Engine e(HostOnly{}, arch, weights, num_classes, image_size, options);
  PackDigest d;
  const std::vector<uint8_t> host = e.pack_host(weights, &d.regions);
  d.total = host.size();
  d.arena = fnv1a(host.data(), host.size());
  std::vector<const PackRegion*> by_off;
  for (const PackRegion& r : d.regions) {
    by_off.push_back(&r);
    d.region_digests.push_back(fnv1a(host.data() + r.off, r.bytes));
  }
  std::sort(by_off.begin(), by_off.end(), [](const PackRegion* a, const PackRegion* b) { return a->off < b->off; });
  for (const PackRegion* r : by_off) {
    uint64_t& h = d.kinds.emplace(r->kind, kFnvBasis).first->second;
    h = fnv1a(host.data() + r->off, r->bytes, h);
  }
  for (const ConvLayer& L : e.convs_) d.orders.emplace_back(L.name, frag_order_name(L.frag));
  return d;
}

}  // namespace dmlc
