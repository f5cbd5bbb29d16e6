// Query-batch e4m3 3x3/p1 conv (B <= a few images), stride 1 or 2, e4m3 in and
// out, on the block-scaled e4m3 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, unit
// block scales): the e4m3 3x3 convs of resnet18_fp8 / resnet34_fp8 (layers 3-4,
// with the e4m3 residual and layer4.0's fused 1x1/s2 downsample) and of
// resnet50_fp8 (the bottleneck 3x3s of layers 2-4) at the serving fleet's
// batch-1 query shape.
//
// Reference equivalent: BasicBlock.conv1/conv2 (+ downsample) and
// Bottleneck.conv2 of tch::vision::resnet18/34/50, run for ONE image per query
// by `forward_t`. conv3x3_stream8 gives a workgroup whole images, so at B = 1
// it would light 1-4 CUs; the e4m3 implicit GEMM has 128x128 / 256x64 tiles and
// no split-K, so M = 49..196 pixels against K = 2304..4608 is a handful of
// workgroups walking K alone. Here, as in conv_small.hip (the bf16 kernel this
// one mirrors), one launch per conv, no split-K workspace, no second kernel:
//
//  * grid = (CO/16 channel tiles, pixel tiles of MF x 16 output pixels, B). A
//    channel tile is ONE 16-row N fragment nf of a 32-channel group g of the
//    stream8 fragment-order weights (conv3x3_stream8_frag_offset), so a lane
//    ends with the 4 consecutive channels 32g + 8fq + 4nf .. +3 of one pixel
//    (4-B stores). One fragment and not the whole group: at B = 1 the grid is
//    what puts CUs to work (7x7x512: 128 workgroups instead of 64), a workgroup
//    streams half the weight bytes (73 KB instead of 147 KB at K = 4608, the
//    longest dependent wait of the kernel), and 9 K-tiles per wave stay 72
//    weight VGPRs. The price, the X fragments read from LDS once per N fragment
//    on two CUs instead of once, is LDS bandwidth nobody else wants here;
//  * the input rows a pixel tile reads (all columns, all channels, CI bytes a
//    pixel) go to LDS once by LDS-DMA. Staged position: row-major, and at
//    stride 2 each row's even columns first, then its odd ones, so the 16
//    pixels of a fragment sit at consecutive positions for every tap (as in
//    conv3x3_stream8_kernel.h). A pixel's 32-B chunk pair m sits at physical
//    pair m ^ (pos & 7) (128-B pixels: m ^ ((pos >> 1) & 3), the position's
//    parity picking the half of the 256-B bank window), each chunk keeping its
//    half; lanes with odd fq read their pair's second chunk first, as the
//    weights are packed: each lane's two ds_read_b128 of 32 consecutive
//    channels are bank-conflict free along a fragment;
//  * padding taps (and the pixels past the end of the last tile) read a zero
//    chunk by address select;
//  * the 4 waves split the K-tiles (wave w: t = w, w + 4, ...; a K-tile is one
//    tap's 128 input channels) and load ALL their weight fragments into
//    registers straight after the input DMA (<= 9 tiles x 2 halves x 16 B per
//    lane): every global load of the kernel is in flight at once;
//  * DS (stride 2): the 1x1/s2 downsample reads exactly the centre tap's
//    input, so its K-tile cc is the centre tap's K-tile against wd, into a
//    second accumulator, with no extra LDS reads. The centre tap's tiles are
//    t = 4 CT + cc = cc (mod 4): wave cc owns downsample tile cc, at its step
//    j = CT;
//  * the waves' fp32 partial sums meet in LDS and are added in wave order
//    0..3; wave f then finishes pixel fragment f: q = fma(acc, alpha inv, bias
//    inv), RES: q = fma(f32(res), res_scale inv, q), y = e4m3(med3(q, relu ? 0
//    : -448, 448)); yd the same with its own operands and no ReLU
//    (conv3x3_stream8_kernel.h's arithmetic).
//
// Compiled without packed fp32 VALU ops (tools/build.py).
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace dmlc {

namespace {

struct Small8Args {
  const uint8_t* x;     // [B, H, W, CI] e4m3
  const uint8_t* wf;    // [CO/32][9 CI/128][2 nf][2 h][64][16] (conv3x3_stream8_frag_offset)
  const float* alpha;   // [CO]
  const float* bias;    // [CO]
  const uint8_t* res;   // [B, Ho, Wo, CO] e4m3 or null
  uint8_t* y;           // [B, Ho, Wo, CO] e4m3
  const uint8_t* zero;  // >= 16 zero bytes
  const uint8_t* wd;    // DS: [CO/32][CI/128][2][2][64][16]
  const float* alpha_d;
  const float* bias_d;
  uint8_t* yd;          // DS: [B, Ho, Wo, CO] e4m3
  int H, W, Ho, Wo, CO;
  float lo_clamp;       // relu ? 0 : -448
  float inv, res_scale, inv_d;
};

// chunk-pair key of staged position k (see the header)
template <int CI>
__device__ __forceinline__ int pair_key(int k) {
  return CI >= 256 ? (k & 7) : ((k >> 1) & 3);
}

template <int MF, bool DS>
constexpr int part_bytes() {
  return 4 * MF * 64 * 16 * (DS ? 2 : 1);
}
constexpr int kZeroBytes = 256;  // the zero chunk; keeps the staged rows on a 256-B bank window

template <int CI, int S, int MF, bool DS>
__global__ __launch_bounds__(256, 1) void conv_small8_kernel(Small8Args a) {
  constexpr int CPX = CI / 16;      // 16-B chunks per staged pixel
  constexpr int CT = CI / 128;      // K-tiles per tap
  constexpr int KT = 9 * CT;        // K-tiles
  constexpr int KW = (KT + 3) / 4;  // K-tiles per wave (at most)
  constexpr int PART = part_bytes<MF, DS>();
  constexpr int ZOFF = PART;               // 16 zero bytes
  constexpr int ROFF = PART + kZeroBytes;  // staged input rows
  static_assert(CT == 1 || CT == 2 || CT == 4, "a wave owns at most one downsample K-tile");
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  char* lds = (char*)smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int g = blockIdx.x >> 1, nf = blockIdx.x & 1;
  const int b = blockIdx.z;
  const int H = a.H, W = a.W, Wo = a.Wo;
  const int We = (W + 1) >> 1;  // stride 2: a staged row's even columns come first
  const int P = a.Ho * Wo;
  const int p0 = blockIdx.y * (MF * 16);
  const int p1 = min(p0 + MF * 16, P);
  const int oh_lo = p0 / Wo, oh_hi = (p1 - 1) / Wo;
  const int ih_lo = max(0, oh_lo * S - 1), ih_hi = min(H - 1, oh_hi * S + 1);
  const int total = (ih_hi - ih_lo + 1) * W * CPX;  // staged chunks

  // ---- input rows ih_lo..ih_hi -> LDS: physical chunk pc of position pos
  // holds logical chunk ((pc >> 1) ^ key(pos)) << 1 | (pc & 1)
  {
    const uint8_t* src0 = a.x + ((long)b * H + ih_lo) * W * CI;
    char* reg = lds + ROFF;
    for (int s0 = wave * 64; s0 < total; s0 += 256) {
      const int s = s0 + lane;
      if (s < total) {
        const int pos = s / CPX, pc = s - pos * CPX;
        const int r = pos / W, xp = pos - r * W;
        const int xc = S == 1 ? xp : (xp < We ? 2 * xp : 2 * (xp - We) + 1);
        const int lc = (((pc >> 1) ^ pair_key<CI>(pos)) << 1) | (pc & 1);
        dma16(src0 + ((long)r * W + xc) * CI + 16 * lc, reg + s0 * 16);
      }
    }
  }
  if (tid == 0) dma16(a.zero, lds + ZOFF);

  // ---- this wave's weight fragments: K-tiles t = wave + 4 j (4 KB a tile and
  // group: [nf][h][lane][16])
  const uint8_t* wb = a.wf + (long)g * KT * 4096 + nf * 2048 + lane * 16;
  v8i wr[KW];
#pragma unroll
  for (int j = 0; j < KW; ++j) {
    const int t = wave + 4 * j;
    if (KT % 4 == 0 || t < KT)
      wr[j] = e4m3x32(*(const uint4*)(wb + (long)t * 4096), *(const uint4*)(wb + (long)t * 4096 + 1024));
  }
  v8i wdr = {0, 0, 0, 0, 0, 0, 0, 0};
  if constexpr (DS) {
    if (wave < CT) {
      const uint8_t* wdb = a.wd + ((long)g * CT + wave) * 4096 + nf * 2048 + lane * 16;
      wdr = e4m3x32(*(const uint4*)wdb, *(const uint4*)(wdb + 1024));
    }
  }

  // ---- per-lane pixel geometry: staged position of tap (0, 0) (stride 2: of
  // the even column ow, the column part of every tap's offset below) and the
  // taps inside the image (bit kh * 3 + kw)
  int pb[MF], vm[MF];
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    const int p = p0 + 16 * f + fr;
    const int oh = p / Wo, ow = p - (p / Wo) * Wo;
    const int ih = oh * S - 1, iw = ow * S - 1;
    pb[f] = (ih - ih_lo) * W + (S == 1 ? iw : ow);
    int m = 0;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
        m |= ((unsigned)(ih + kh) < (unsigned)H && (unsigned)(iw + kw) < (unsigned)W) << (kh * 3 + kw);
    vm[f] = p < p1 ? m : 0;
  }

  // the input DMA has landed for every wave: only weight loads, issued after
  // it, may still be in flight (vmcnt retires in order). The waves issued
  // unequal numbers of them (KT = 9, 18; the downsample's): wait for the
  // smallest, 2 loads x KT / 4 tiles
  vm_wait<2 * (KT / 4)>();
  lds_barrier();

  floatx4 acc[MF], accd[MF];
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    acc[f] = floatx4{0.f, 0.f, 0.f, 0.f};
    accd[f] = acc[f];
  }
#pragma unroll
  for (int j = 0; j < KW; ++j) {
    const int t = wave + 4 * j;
    if (KT % 4 != 0 && t >= KT) break;
    const int tap = t / CT, cc = t - tap * CT;
    const int kh = tap / 3, kw = tap - kh * 3;
    const int dpos = kh * W + (S == 1 ? kw : kw == 0 ? We - 1 : kw == 1 ? 0 : We);
    const int m = 4 * cc + fq;  // this lane's logical chunk pair
#pragma unroll
    for (int f = 0; f < MF; ++f) {
      const int pos = pb[f] + dpos;
      const bool ok = (vm[f] >> tap) & 1;
      const int base = ROFF + pos * CI + ((m ^ pair_key<CI>(pos)) << 5) + ((fq & 1) << 4);
      const uint4 lo = *(const uint4*)(lds + (ok ? base : ZOFF));
      const uint4 hi = *(const uint4*)(lds + (ok ? base ^ 16 : ZOFF));
      const v8i xb = e4m3x32(lo, hi);
      acc[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wr[j], xb, acc[f], 0, 0, 0, 127, 0, 127);
      if constexpr (DS) {
        // this wave's centre-tap tile t = 4 CT + wave: downsample K-tile cc = wave
        if (j == CT && wave < CT)
          accd[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wdr, xb, accd[f], 0, 0, 0, 127, 0, 127);
      }
    }
  }

  // ---- the 4 waves' partial sums meet in LDS: [wave][f][lane] (DS: + MF x 4 x 64)
  floatx4* part = (floatx4*)lds;
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    part[(wave * MF + f) * 64 + lane] = acc[f];
    if constexpr (DS) part[(4 * MF + wave * MF + f) * 64 + lane] = accd[f];
  }
  lds_barrier();

  // ---- epilogue: wave f finishes pixel fragment f; the lane's 4 channels
  const int ch = 32 * g + 8 * fq + 4 * nf;
  for (int f = wave; f < MF; f += 4) {
    const int p = p0 + 16 * f + fr;
    if (p >= p1) continue;
    const long o = ((long)b * P + p) * a.CO + ch;
    floatx4 v = part[f * 64 + lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) v += part[(w * MF + f) * 64 + lane];
    float q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = __builtin_fmaf(v[i], a.alpha[ch + i] * a.inv, a.bias[ch + i] * a.inv);
    if (a.res) {
      const float rsi = a.res_scale * a.inv;
      float rv[4];
      e4m3x4_to_f32(*(const uint32_t*)(a.res + o), rv);
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = __builtin_fmaf(rv[i], rsi, q[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = __builtin_amdgcn_fmed3f(q[i], a.lo_clamp, 448.f);
    *(uint32_t*)(a.y + o) = e4m3x4_from_f32(q[0], q[1], q[2], q[3]);
    if constexpr (DS) {
      floatx4 d = part[(4 * MF + f) * 64 + lane];
#pragma unroll
      for (int w = 1; w < 4; ++w) d += part[(4 * MF + w * MF + f) * 64 + lane];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        q[i] = __builtin_amdgcn_fmed3f(__builtin_fmaf(d[i], a.alpha_d[ch + i] * a.inv_d, a.bias_d[ch + i] * a.inv_d),
                                       -448.f, 448.f);
      *(uint32_t*)(a.yd + o) = e4m3x4_from_f32(q[0], q[1], q[2], q[3]);
    }
  }
}

// staged input rows of the worst pixel tile
int max_rows(int H, int Ho, int Wo, int S, int mf) {
  const int P = Ho * Wo, tp = mf * 16;
  int best = 0;
  for (int p0 = 0; p0 < P; p0 += tp) {
    const int p1 = std::min(p0 + tp, P);
    const int lo = std::max(0, (p0 / Wo) * S - 1), hi = std::min(H - 1, ((p1 - 1) / Wo) * S + 1);
    best = std::max(best, hi - lo + 1);
  }
  return best;
}

size_t lds_bytes(int H, int W, int CI, int Ho, int Wo, int S, int mf, bool ds) {
  return (size_t)4 * mf * 64 * 16 * (ds ? 2 : 1) + kZeroBytes + (size_t)max_rows(H, Ho, Wo, S, mf) * W * CI;
}

constexpr size_t kMaxLds = 160 * 1024;

template <int CI, int S, int MF, bool DS>
void launch(const Small8Args& a, int B, size_t lds, hipStream_t s) {
  const dim3 grid(a.CO / 16, (a.Ho * a.Wo + MF * 16 - 1) / (MF * 16), B);
  hipLaunchKernelGGL((conv_small8_kernel<CI, S, MF, DS>), grid, dim3(256), lds, s, a);
}

template <int CI, int S, bool DS>
void launch_mf(const Small8Args& a, int B, int mf, size_t lds, hipStream_t s) {
  switch (mf) {
    case 1: launch<CI, S, 1, DS>(a, B, lds, s); break;
    case 2: launch<CI, S, 2, DS>(a, B, lds, s); break;
    default: launch<CI, S, 4, DS>(a, B, lds, s); break;
  }
}

template <int CI>
void launch_ci(const Small8Args& a, int B, int stride, bool ds, int mf, size_t lds, hipStream_t s) {
  if (stride == 1)
    launch_mf<CI, 1, false>(a, B, mf, lds, s);
  else if (ds)
    launch_mf<CI, 2, true>(a, B, mf, lds, s);
  else
    launch_mf<CI, 2, false>(a, B, mf, lds, s);
}

}  // namespace

bool conv_small8_supported(int H, int W, int CI, int CO, int stride, bool res, bool ds) {
  if (!(CI == 128 || CI == 256 || CI == 512) || (stride != 1 && stride != 2)) return false;
  if (!(CO == CI || (CO == 2 * CI && stride == 2))) return false;
  if (res && (stride != 1 || CO != CI)) return false;
  if (ds && stride != 2) return false;
  if (H <= 0 || W <= 0) return false;
  const int Ho = conv_out_dim(H, 3, stride, 1), Wo = conv_out_dim(W, 3, stride, 1);
  if (Ho <= 0 || Wo <= 0) return false;
  return lds_bytes(H, W, CI, Ho, Wo, stride, 1, ds) <= kMaxLds;
}

int conv_small8_pick_mf(int B, int H, int W, int CI, int CO, int stride, bool ds, int num_cus) {
  const int Ho = conv_out_dim(H, 3, stride, 1), Wo = conv_out_dim(W, 3, stride, 1);
  const int P = Ho * Wo;
  // the widest pixel tile that still gives ~half the CUs a workgroup (fewer,
  // fatter workgroups re-read the weights less often)
  for (int mf : {4, 2}) {
    const long wgs = (long)(CO / 16) * ((P + mf * 16 - 1) / (mf * 16)) * B;
    if (wgs >= num_cus / 2 && lds_bytes(H, W, CI, Ho, Wo, stride, mf, ds) <= kMaxLds) return mf;
  }
  return 1;
}

void conv_small8(const void* x, const void* wf, const float* alpha, const float* bias, void* y, const void* zero,
                 int B, int H, int W, int CI, int CO, int stride, bool relu, float out_inv_scale, int mf,
                 hipStream_t s, const Stream8Block* blk) {
  if (B <= 0) return;
  const void* res = blk ? blk->res : nullptr;
  const bool ds = blk && blk->wd;
  if (!conv_small8_supported(H, W, CI, CO, stride, res != nullptr, ds))
    throw std::invalid_argument("conv_small8: unsupported shape");
  if (!x || !wf || !alpha || !bias || !y || !zero) throw std::invalid_argument("conv_small8: null operand");
  if (((uintptr_t)x | (uintptr_t)wf | (uintptr_t)zero) & 15)
    throw std::invalid_argument("conv_small8: x, wf and zero must be 16-B aligned");
  if ((uintptr_t)y & 3) throw std::invalid_argument("conv_small8: y must be 4-B aligned");
  if (((uintptr_t)alpha | (uintptr_t)bias) & 3) throw std::invalid_argument("conv_small8: alpha / bias misaligned");
  if (!(out_inv_scale > 0.f)) throw std::invalid_argument("conv_small8: no output scale");
  if (mf != 1 && mf != 2 && mf != 4) throw std::invalid_argument("conv_small8: mf must be 1, 2 or 4");
  const int Ho = conv_out_dim(H, 3, stride, 1), Wo = conv_out_dim(W, 3, stride, 1);
  if ((long)B * H * W * CI >= (1L << 31) || (long)B * Ho * Wo * CO >= (1L << 31))
    throw std::invalid_argument("conv_small8: tensor too large for 32-bit offsets");
  if (B > 65535) throw std::invalid_argument("conv_small8: batch too large");
  const size_t xn = (size_t)B * H * W * CI, yn = (size_t)B * Ho * Wo * CO;
  if (ranges_overlap(x, xn, y, yn)) throw std::invalid_argument("conv_small8: in-place not supported");
  if (res && (((uintptr_t)res & 3) || ranges_overlap(res, yn, y, yn) || ranges_overlap(res, yn, x, xn)))
    throw std::invalid_argument("conv_small8: res is misaligned or overlaps x / y");
  if (ds && (!blk->alpha_d || !blk->bias_d || !blk->yd || ((uintptr_t)blk->wd & 15) || ((uintptr_t)blk->yd & 3) ||
             (((uintptr_t)blk->alpha_d | (uintptr_t)blk->bias_d) & 3) || !(blk->out_inv_scale_d > 0.f) ||
             ranges_overlap(blk->yd, yn, y, yn) || ranges_overlap(blk->yd, yn, x, xn)))
    throw std::invalid_argument("conv_small8: null / misaligned downsample operand, no scale, or yd overlaps x / y");
  const size_t lds = lds_bytes(H, W, CI, Ho, Wo, stride, mf, ds);
  if (lds > kMaxLds) throw std::invalid_argument("conv_small8: pixel tile too large for LDS");
  Small8Args a;
  a.x = (const uint8_t*)x;
  a.wf = (const uint8_t*)wf;
  a.alpha = alpha;
  a.bias = bias;
  a.res = (const uint8_t*)res;
  a.y = (uint8_t*)y;
  a.zero = (const uint8_t*)zero;
  a.wd = ds ? (const uint8_t*)blk->wd : nullptr;
  a.alpha_d = ds ? blk->alpha_d : nullptr;
  a.bias_d = ds ? blk->bias_d : nullptr;
  a.yd = ds ? (uint8_t*)blk->yd : nullptr;
  a.H = H;
  a.W = W;
  a.Ho = Ho;
  a.Wo = Wo;
  a.CO = CO;
  a.lo_clamp = relu ? 0.f : -448.f;
  a.inv = out_inv_scale;
  a.res_scale = res ? blk->res_scale : 0.f;
  a.inv_d = ds ? blk->out_inv_scale_d : 0.f;
  switch (CI) {
    case 128: launch_ci<128>(a, B, stride, ds, mf, lds, s); break;
    case 256: launch_ci<256>(a, B, stride, ds, mf, lds, s); break;
    default: launch_ci<512>(a, B, stride, ds, mf, lds, s); break;
  }
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
