// Direct 3x3 / stride 1 / pad 1 convolution on the block-scaled e4m3 MFMA
// (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales), e4m3 in and out:
// ResNet50's bottleneck 3x3 convs of layer2 (28x28x128), layer3 (14x14x256)
// and layer4 (7x7x512), whose input t1 comes from the reduce 1x1 conv and
// whose output t2 feeds the e4m3 expand conv (resnet50_fp8,
// EngineOptions::fp8_3x3_in).
//
// Reference equivalent: Bottleneck.conv2 + bn2 + relu of tch::vision::resnet50
// (BASELINE config 5: the model zoo path of src/services.rs:513-524, run per
// query by `forward_t` at :493). These convs are ~45% of ResNet50's FLOPs; on
// bf16 MFMA (conv3x3_stream.hip) they ran 51-54 us each at B = 256. Here the
// same structure runs at the e4m3 rate (a 16x16x128 MFMA = 2x the bf16 FLOPs
// per cycle) with half the staged bytes:
//
//  * a workgroup owns IMG whole images (resident in LDS, e4m3: 49 KB for a
//    14x14x256 image) and CO / NSP output channels; 8 waves (2 per SIMD) =
//    WM pixel groups x 8 / WM channel groups of 32 NG channels;
//  * every wave streams the fragment-order e4m3 weights of its channels from
//    L2 into a PD-deep register ring (no LDS stage, no barrier in the K loop);
//    a K-tile is one tap's 128 input channels (one MFMA k-step);
//  * D = W x X: lane (fr, fq) of an X fragment holds 32 consecutive input
//    channels of pixel fr (two 16-B LDS reads). A 16-B chunk pair of a
//    staged pixel sits at pair index m ^ (K & 7) (K = the staged pixel's
//    index, consecutive along a fragment), and lanes with odd fq read their
//    pair's second chunk first (their weight fragments are packed with the
//    same half swap, so the dot product is unchanged): in every 16-lane
//    group of a ds_read_b128 the 8 lanes of one fq read 8 distinct pairs and
//    the two fq take opposite halves, so the reads are bank-conflict free
//    (tests/test_layouts_cpu.py). 128-channel pixels (128 B, half a bank
//    row) key the pair by (K >> 1) & 3 instead: K's parity picks the window
//    half, and the 8 lanes of one fq (4 + 4 consecutive K, or 8) cover the 8
//    values of K & 7 once;
//  * epilogue: v = acc * alpha[n] + bias[n] (alpha = the per-channel e4m3
//    weight scale x the input scale; t2's per-channel output scales are
//    folded into both), ReLU, e4m3 (saturated at 448), 8 consecutive
//    channels of a pixel per 8-B store.
//
// The basic-block forms (ResNet18 / 34 layers 3-4, conv3x3_stream8_block.hip):
//  * RES: the epilogue adds an e4m3 residual, the 8 bytes per (pixel
//    fragment, channel group) that the lane later stores; they are loaded at
//    the start of the last K-tile but one, so they land under the last
//    MFMAs, and are waited for where the epilogue first uses them;
//  * WIDE (CO = 2 CI at stride 2) is the CO == 8 / WM * WN * NSP split with
//    KT = 9 CI / 128;
//  * DS: a second phase after the 3x3's epilogue computes the block's 1x1/s2
//    downsample from the resident input: input pixel (2y, 2x) is the 3x3's
//    centre tap (set_tap(4), which never selects the zero pixel), so the same
//    accumulators, zeroed, take CI / 128 more K-tiles against wd (the same
//    fragment order, KT = CI / 128; they fit the weight ring, free by then,
//    and are loaded under the first epilogue's stores) and a second epilogue
//    without ReLU writes yd.
//
// This header is the kernel template; conv3x3_stream8.hip instantiates the
// ResNet50 forms, conv3x3_stream8_block.hip the basic-block forms.
#pragma once
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace dmlc {

struct Stream8Args {
  const uint8_t* x;     // [B, H, W, CI] e4m3
  const uint8_t* wf;    // e4m3 weights in stream8 fragment order (conv3x3_stream8_frag_offset)
  const float* alpha;   // [CO]: dequantisation of acc (input scale x weight scale)
  const float* bias;    // [CO]
  uint8_t* y;           // [B, H, W, CO] e4m3
  const uint8_t* zero;  // >= 16 zero bytes
  int B;
  int relu;
  float out_inv_scale;  // y = e4m3(relu(v) * out_inv_scale)
  int stagger;          // start_stagger (common.h)
};

// The basic-block forms' kernel argument (RES / DS instantiations only: the
// other forms keep Stream8Args as their kernarg)
struct Stream8BlockArgs : Stream8Args {
  const uint8_t* res = nullptr;   // RES: [B, H, W, CO] e4m3, 8-B aligned
  float res_scale = 0.f;          // y = e4m3(relu(v + res * res_scale) * out_inv_scale)
  float out_inv_scale_d = 0.f;    // DS: yd = e4m3((acc_d * alpha_d + bias_d) * out_inv_scale_d), no ReLU
  const uint8_t* wd = nullptr;    // DS: e4m3 [CO][CI] in the same fragment order, KT = CI / 128 (null: the conv alone)
  const float* alpha_d = nullptr;
  const float* bias_d = nullptr;
  uint8_t* yd = nullptr;          // [B, H, W, CO] e4m3
};

// The basic-block forms' launch (conv3x3_stream8_block.hip); the caller has
// checked conv3x3_stream8_block_supported and the operands.
void conv3x3_stream8_block_launch(const Stream8BlockArgs& a, int Cin, int stride, hipStream_t s);

namespace {

// Geometry: output H x W, stride S; a workgroup owns HS output rows of one
// image (PARTS = H / HS > 1: stride 2, or two halves at stride 1) or IMG
// whole images.
template <int H, int W, int CI, int HS, int IMG, int S>
struct Stream8Geom {
  static constexpr int PARTS = H / HS;
  static_assert(PARTS == 1 || IMG == 1, "strips: one image");
  static constexpr int HI = S * H, WI = S * W;   // input rows / columns
  // staged rows: whole images, the strip's input rows 2 r0 - 1 .. 2 (r0 +
  // HS - 1) + 1 (stride 2 never reads below the image), or a strip and its
  // halo rows inside the image (stride 1)
  static constexpr int XR = PARTS == 1 ? IMG * HI
                            : S == 1   ? HS + (PARTS > 2 ? 2 : 1)
                                       : (S * (HS - 1) + 3 < HI ? S * (HS - 1) + 3 : HI);
  static constexpr int PXB = CI;                 // bytes per staged pixel
  static constexpr int ROWB = WI * PXB;
  static constexpr int ZB = XR * ROWB;           // the zero pixel
  // (128-B pixels: two zero pixels, the window half a real pixel of the same
  // K parity would use, so border lanes keep their bank slots)
  static constexpr int ZBYTES = PXB >= 256 ? PXB : 256;
  static constexpr int LDS = ZB + ZBYTES;
  static constexpr int CH = XR * WI * (CI / 16);  // 16-B chunks staged (at most)
};

template <int H, int W, int CI, int CO, int HS, int IMG, int NSP, int WM, int NG, int PD, int S, bool RES = false,
          bool DS = false>
__global__ __launch_bounds__(512, 1) void conv3x3_stream8_kernel(
    std::conditional_t<RES || DS, Stream8BlockArgs, Stream8Args> a) {
  using G = Stream8Geom<H, W, CI, HS, IMG, S>;
  constexpr int PARTS = G::PARTS, HI = G::HI, WI = G::WI;
  constexpr int NPIX = IMG * HS * W;         // output pixels per workgroup
  constexpr int MFT = (NPIX + 15) / 16;      // pixel fragments (the last one partly padding)
  constexpr int MF = (MFT + WM - 1) / WM;    // per wave
  constexpr int WN = 32 * NG;                // channels per wave
  constexpr int NF = 2 * NG;                 // N fragments per wave
  constexpr int CT = CI / 128;               // K-tiles per tap
  constexpr int KT = 9 * CT;                 // K-tiles
  constexpr int CPX = CI / 16;               // 16-B chunks per pixel
  static_assert(CO == 8 / WM * WN * NSP, "channel split");
  static_assert(CI % 128 == 0 && (CPX >= 16 || CPX == 8), "e4m3 pixels of 128 B or >= 256 B (whole bank rows)");
  // ring slot of K-tile t = tap * CT + cc: cc % PD (tap loop rolled), or t % PD
  // (CT = 1: the 9 taps unrolled): compile-time register indices either way
  static_assert(CT == 1 || CT % PD == 0, "weight ring depth");
  static_assert(G::LDS <= 160 * 1024, "LDS budget");
  static_assert(S == 1 || (S == 2 && WI % 2 == 0), "stride");
  static_assert(!RES || (S == 1 && CI == CO), "RES: an identity block's second conv");
  static_assert(!DS || (S == 2 && PARTS == 1 && CT <= PD), "DS: the centre tap of whole resident images");

  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  char* xs = (char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  start_stagger(a.stagger);
  const int wm = wave % WM, wc = wave / WM;
  const int fr = lane & 15, fq = lane >> 4;
  const int ns = blockIdx.x % NSP, rest = blockIdx.x / NSP;
  const int bg = rest / PARTS, part = rest - bg * PARTS;
  const int b = bg * IMG, nimg = min(IMG, a.B - b);
  const int r0 = part * HS;                                  // first output row
  const int rs = PARTS == 1 ? 0 : max(S * r0 - 1, 0);        // first staged input row
  const int nrows = PARTS == 1 ? nimg * HI : min(S * (r0 + HS - 1) + 1, HI - 1) - rs + 1;
  const int npix = IMG == 1 ? NPIX : nimg * HS * W;
  const int ch0 = ns * (CO / NSP) + wc * WN;
  const uint8_t* img = a.x + (long)b * HI * WI * CI;
  // chunk-pair key of staged pixel K (see the header)
  auto pswz = [](int k) __attribute__((always_inline)) { return CPX >= 16 ? (k & 7) : ((k >> 1) & 3); };

  // ---- stage the input rows (one flat run of 16-B chunks; stride 2: each
  // row's even columns first, then its odd ones). The key K of a staged
  // pixel is chosen so that for output pixel p at tap (kh, kw) it is p + a
  // tap constant, consecutive along a fragment even where it wraps a row:
  //   stride 1 (whole images): K = staged row * W + x;
  //   stride 2: K = image * H * W + (((y + 1) >> 1) - r0) * W + ((x + 1) >> 1).
  // Logical chunk pair m of a staged pixel sits at physical pair m ^ (K & 7),
  // each chunk keeping its half.
  for (int k0 = wave * 64; k0 < G::CH; k0 += 512) {
    const int ci = k0 + lane;
    const int i = ci / (WI * CPX), rem = ci - i * (WI * CPX);
    const int q = rem / CPX, pc = rem - q * CPX;  // physical column, chunk
    const int x = S == 1 ? q : (q < WI / 2 ? 2 * q : 2 * (q - WI / 2) + 1);
    int K;
    if constexpr (S == 1) {
      K = i * W + x;
    } else {
      const int ii = PARTS == 1 ? i / HI : 0, y = PARTS == 1 ? i - ii * HI : rs + i;
      K = ii * (H * W) + (((y + 1) >> 1) - r0) * W + ((x + 1) >> 1);
    }
    const int lc = ((((pc >> 1) ^ pswz(K)) << 1) | (pc & 1));  // logical chunk at physical pc
    const uint8_t* src = i < nrows ? img + ((long)(rs + i) * WI + x) * CI + 16 * lc : a.zero;
    if (G::CH % 64 == 0 || ci < G::CH) dma16(src, xs + k0 * 16);
  }
  if (wave == 0 && lane < G::ZBYTES / 16) dma16(a.zero, xs + G::ZB);

  // ---- weights: fragment (group j, K-tile t, nf, half h) = 1 KB, lane l's
  // 16 B at l * 16 (conv3x3_stream8_frag_offset); this wave's NG groups are
  // consecutive
  const __amdgpu_buffer_rsrc_t wrs = wave_rsrc(a.wf + (long)(ch0 / 32) * KT * 4 * 1024, NG * KT * 4 * 1024);
  auto wfrag = [&](int t, int nf) __attribute__((always_inline)) {
    const int base = (((nf >> 1) * KT + t) * 2 + (nf & 1)) * 2 * 1024;
    const uint4 lo = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(wrs, lane * 16, base, 0));
    const uint4 hi = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(wrs, lane * 16, base + 1024, 0));
    return v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  };
  v8i wq[PD][NF];
#pragma unroll
  for (int t = 0; t < PD - 1; ++t)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) wq[t][nf] = wfrag(t, nf);

  // ---- per-lane pixel constants: xoff = the staged offset of the tap-(1,1)
  // input pixel | flags for the image's first / last row and column (their
  // outside taps read the zero pixel; stride 2 never leaves the image at the
  // bottom or right)
  int xoff[MF];
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    const int p = min(16 * (wm * MF + f) + fr, npix - 1);
    const int pi = p % (HS * W), ii = p / (HS * W), prow = pi / W, pcol = pi - prow * W, r = r0 + prow;
    const int row = ii * HI + S * r - rs;  // (stride 2: even input column 2 pcol sits at slot pcol)
    xoff[f] = (row * WI + pcol) * G::PXB | (r == 0 ? 1 : 0) | (S == 1 && r == H - 1 ? 2 : 0) | (pcol == 0 ? 4 : 0) |
              (S == 1 && pcol == W - 1 ? 8 : 0);
    asm volatile("" : "+v"(xoff[f]));
  }
  floatx4 acc[MF][NF];
#pragma unroll
  for (int f = 0; f < MF; ++f)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[f][nf] = floatx4{0.f, 0.f, 0.f, 0.f};

  // tap (kh, kw): fragment bases xa[f]; lane offsets of the two reads: pair
  // ((fq + 4 cc) ^ pswz(K)) with K = p + kb + ktap (p & 15 == fr for real
  // pixels; kb: a stride-1 half image's staged rows start r0 - rs rows above
  // its first output row), first the half fq & 1, then the other
  const int kb = S == 1 ? (r0 - rs) * W : 0;
  int xa[MF], tsw0 = 0, tsw1 = 0;
  auto set_tap = [&](int tap) __attribute__((always_inline)) {
    const int kh = tap / 3, kw = tap - kh * 3;
    const int tm = (kh == 0 ? 1 : 0) | (kh == 2 ? 2 : 0) | (kw == 0 ? 4 : 0) | (kw == 2 ? 8 : 0);
    // staged column offset of tap column kw (stride 2: odd columns start at WI / 2)
    const int dq = S == 1 ? kw - 1 : (kw == 0 ? WI / 2 - 1 : kw == 1 ? 0 : WI / 2);
    const int toff = ((kh - 1) * WI + dq) * G::PXB;
    const int ktap = S == 1 ? (kh - 1) * W + (kw - 1) : (kh == 2 ? W : 0) + (kw == 2 ? 1 : 0);
    // 128-B pixels: a real pixel's window half is its staged column's parity,
    // K's parity (stride 2: flipped for kw != 1, the odd columns staged after
    // the even ones); border lanes read the zero pixel in that half, so they
    // keep the bank slots the swizzle gives their K
    const int zh = CPX >= 16 ? 0 : (((fr + kb + ktap) & 1) ^ (S == 2 && kw != 1 ? 1 : 0));
#pragma unroll
    for (int f = 0; f < MF; ++f) xa[f] = (xoff[f] & tm) ? G::ZB + zh * 128 : (xoff[f] & ~15) + toff;
    const int u = fq ^ pswz(fr + kb + ktap);
    tsw0 = (u << 5) | ((fq & 1) << 4);
    tsw1 = tsw0 ^ 16;
  };
  auto xread = [&](int f, int cc) __attribute__((always_inline)) {
    const uint4 lo = *(const uint4*)(xs + xa[f] + (tsw0 ^ (cc << 7)));
    const uint4 hi = *(const uint4*)(xs + xa[f] + (tsw1 ^ (cc << 7)));
    return v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  };

  set_tap(0);
  vm_wait<0>();                  // own input DMAs (and the first weights)
  __builtin_amdgcn_s_barrier();  // everyone's
  asm volatile("" ::: "memory");
  v8i xf[MF];
#pragma unroll
  for (int f = 0; f < MF; ++f) xf[f] = xread(f, 0);
  // RES: the lane's residual bytes, those of its stores (padding lanes read
  // the last real pixel's)
  uint2 rres[RES ? MF : 1][NG];
  // K-tile t = tap * CT + cc, its weights in ring slot `slot`
  auto ktile = [&](const int tap, const int cc, const int slot) __attribute__((always_inline)) {
    const int t = tap * CT + cc;
    if constexpr (RES)
      if (t == KT - 2)
#pragma unroll
        for (int f = 0; f < MF; ++f)
#pragma unroll
          for (int j = 0; j < NG; ++j)
            rres[f][j] = *(const uint2*)(a.res + ((long)b * H + r0) * W * CO + ch0 + 8 * fq + 32 * j +
                                         (long)min(16 * (wm * MF + f) + fr, npix - 1) * CO);
    if (t + PD - 1 < KT)
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) wq[(slot + PD - 1) % PD][nf] = wfrag(t + PD - 1, nf);
    if (cc + 1 == CT && tap + 1 < 9) set_tap(tap + 1);
    const int cn = cc + 1 == CT ? 0 : cc + 1;
    __builtin_amdgcn_s_waitcnt(0xC07F);  // the X fragments read during the previous K-tile
#pragma unroll
    for (int f = 0; f < MF; ++f) {
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        acc[f][nf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wq[slot][nf], xf[f], acc[f][nf], 0, 0, 0, 127,
                                                                       0, 127);
      if (t + 1 < KT) xf[f] = xread(f, cn);
    }
#pragma unroll
    for (int f = 0; f < MF; ++f) {
      __builtin_amdgcn_sched_group_barrier(0x008, NF, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
  };
  if constexpr (CT == 1) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) ktile(tap, 0, tap % PD);
  } else {
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int cc = 0; cc < CT; ++cc) ktile(tap, cc, cc % PD);
  }

  // every MFMA done here: pinned, the compiler cannot sink the last K-tile's
  // MFMA chains into the pixel-conditional stores below (their operands then
  // stay live across the whole epilogue and spill)
#pragma unroll
  for (int f = 0; f < MF; ++f)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) asm volatile("" : "+v"(acc[f][nf]));
  // ---- epilogue: lane holds channels ch0 + 32 j + 8 fq .. +7 of its pixel.
  // The 1 / s_out quantisation scale (> 0) is folded into alpha and the bias,
  // so a value costs half a v_pk_fma_f32 (channel pairs sit in consecutive
  // accumulator registers) and one med3 (ReLU and the +-448 saturation
  // together). RES: q = fma(f32(res), res_scale * inv, q) before the med3.
  auto epilogue = [&](const float* alpha, const float* bias, const float inv, const float lo_clamp, uint8_t* y)
      __attribute__((always_inline)) {
    f32x2 al[NG][4], bs[NG][4];
#pragma unroll
    for (int j = 0; j < NG; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = ch0 + 32 * j + 8 * fq + 2 * e;
        al[j][e] = f32x2{alpha[c], alpha[c + 1]} * inv;
        bs[j][e] = f32x2{bias[c], bias[c + 1]} * inv;
      }
    const long base = ((long)b * H + r0) * W * CO + ch0 + 8 * fq;
#pragma unroll
    for (int f = 0; f < MF; ++f) {
      const int p = 16 * (wm * MF + f) + fr;
      if (p >= npix) continue;
#pragma unroll
      for (int j = 0; j < NG; ++j) {
        float q[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const floatx4& ac = acc[f][2 * j + (e >> 1)];
          const f32x2 r = __builtin_elementwise_fma(f32x2{ac[2 * (e & 1)], ac[2 * (e & 1) + 1]}, al[j][e], bs[j][e]);
          q[2 * e] = r.x;
          q[2 * e + 1] = r.y;
        }
        if constexpr (RES) {
          const float rsi = a.res_scale * inv;
          float rv[8];
          e4m3x4_to_f32(rres[f][j].x, rv);
          e4m3x4_to_f32(rres[f][j].y, rv + 4);
#pragma unroll
          for (int e = 0; e < 8; ++e) q[e] = __builtin_fmaf(rv[e], rsi, q[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = __builtin_amdgcn_fmed3f(q[e], lo_clamp, 448.f);
        *(uint2*)(y + base + 32 * j + (long)p * CO) =
            make_uint2(e4m3x4_from_f32(q[0], q[1], q[2], q[3]), e4m3x4_from_f32(q[4], q[5], q[6], q[7]));
      }
    }
  };
  if constexpr (!DS) {
    epilogue(a.alpha, a.bias, a.out_inv_scale, a.relu ? 0.f : -448.f, a.y);
  } else {
    // ---- DS: the 1x1/s2 downsample as a second phase over the centre tap
    // (see the header). All its CT K-tiles fit the ring, free by now: loaded
    // here, they land under the first epilogue's stores.
    const bool ds = a.wd != nullptr;
    if (ds) {
      const __amdgpu_buffer_rsrc_t drs = wave_rsrc(a.wd + (long)(ch0 / 32) * CT * 4 * 1024, NG * CT * 4 * 1024);
#pragma unroll
      for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
          const int o = (((nf >> 1) * CT + t) * 2 + (nf & 1)) * 2 * 1024;
          const uint4 lo = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(drs, lane * 16, o, 0));
          const uint4 hi = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(drs, lane * 16, o + 1024, 0));
          wq[t][nf] = v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        }
      set_tap(4);
#pragma unroll
      for (int f = 0; f < MF; ++f) xf[f] = xread(f, 0);
    }
    epilogue(a.alpha, a.bias, a.out_inv_scale, a.relu ? 0.f : -448.f, a.y);
    if (ds) {
#pragma unroll
      for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) acc[f][nf] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int cc = 0; cc < CT; ++cc) {
        __builtin_amdgcn_s_waitcnt(0xC07F);  // the X fragments
#pragma unroll
        for (int f = 0; f < MF; ++f) {
#pragma unroll
          for (int nf = 0; nf < NF; ++nf)
            acc[f][nf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wq[cc][nf], xf[f], acc[f][nf], 0, 0, 0, 127,
                                                                           0, 127);
          if (cc + 1 < CT) xf[f] = xread(f, cc + 1);
        }
      }
      epilogue(a.alpha_d, a.bias_d, a.out_inv_scale_d, -448.f, a.yd);
    }
  }
}

template <int H, int W, int CI, int CO, int HS, int IMG, int NSP, int WM, int NG, int PD, int S, bool RES = false,
          bool DS = false>
void launch8(const std::conditional_t<RES || DS, Stream8BlockArgs, Stream8Args>& a, hipStream_t s) {
  using G = Stream8Geom<H, W, CI, HS, IMG, S>;
  const int grid = (a.B + IMG - 1) / IMG * (H / HS) * NSP;
  hipLaunchKernelGGL((conv3x3_stream8_kernel<H, W, CI, CO, HS, IMG, NSP, WM, NG, PD, S, RES, DS>), dim3(grid),
                     dim3(512), (size_t)G::LDS, s, a);
}

}  // namespace

}  // namespace dmlc
