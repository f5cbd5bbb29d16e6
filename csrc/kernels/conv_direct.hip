// Direct stride-1 convolutions with the whole input image resident in LDS,
// bias (+ ReLU), bf16 NHWC in and out: AlexNet features.3 (5x5 / pad 2 on
// 27x27x64 -> 192) and features.6 / .8 / .10 (3x3 / pad 1 on 13x13x192 ->
// 384, 384 -> 256, 256 -> 256), each optionally with the 3x3/s2 max-pool that
// follows it (features.5, features.12).
//
// Reference equivalent: those Conv2d + ReLU (+ MaxPool2d) modules of
// tch::vision::alexnet, run per query by `forward_t` (src/services.rs:493).
// As implicit-GEMM tiles (conv_igemm.hip) every tile re-gathers its windows
// through L2: the three 13x13 convs ran at 680-870 TFLOP/s (66 / 105 / 75 us
// at B=256, profiles/r3_alexnet_ops_blaslt.txt) and the 5x5 was AlexNet's
// largest kernel (146-161 us, profiles/r3_alexnet_direct13.txt). Here one
// workgroup = one image, one template kernel over a shape trait:
//
//  * the image goes HBM -> LDS once by LDS-DMA, its 16-B chunks XOR-swizzled
//    per pixel (xswz, common.h: every 16-lane group of a fragment read hits 16
//    distinct bank slots; tests/test_layouts_cpu.py); pixels of more than
//    128 B are padded to a multiple of 256 B; taps outside the image read one
//    zero pixel;
//  * a wave holds FPW pixel fragments x GPP 32-channel groups of accumulators
//    per pass (2 N fragments per group, perm32 row order: a lane ends with 8
//    consecutive channels of one pixel); the weights stream from L2 in
//    fragment order (frag_load, common.h) through a PD-deep register ring, no
//    LDS stage and no barrier in the K loop;
//  * 13x13 (169 pixels, 75-130 KB): 4 waves, one per SIMD with up to 512
//    registers each, split the channels: a wave owns Cout/4 channels for all
//    11 pixel fragments, so each weight fragment feeds 11 MFMAs and each X
//    fragment 4-6. (8 waves of 256 registers spilled the ring: the compiler
//    double-buffers the X fragments.)
//  * 27x27 (729 pixels x 128 B = 93 KB): 8 waves (2 per SIMD) split the pixel
//    fragments: wave w owns fragments 6w .. 6w+5 (46 real; the last wave's 2
//    extra duplicate pixel 728 and are never stored) for all 192 channels, in
//    3 passes of 64 (each X fragment read feeds 4 MFMAs, each weight fragment
//    6; the 8 waves fetch the same weight fragments, mostly L1 hits). (4 waves
//    of 12 fragments at 512 registers: accumulators bounced between VGPRs and
//    AGPRs every K step.)
#include "common.h"
#include "kernels.h"

#include <string>

namespace dmlc {

namespace {

enum class Split { Channels, Fragments };     // what the waves of a workgroup divide among them
enum class Pool { None, PerWave, PerGroup };  // how the fused max-pool's LDS tile is shared

// A shape trait carries only what cannot be derived (DirectGeom derives the
// rest). Each shape keeps its own argument struct: a shared one moves the
// kernarg loads and with them the register allocation.
struct Args13 {
  const bf16* x;      // [B, 13, 13, CI]
  const bf16* wf;     // [CO/32][KT][2][64][8] fragment order (stream_frag_index, K = 9 CI)
  const float* bias;  // [CO]
  bf16* y;            // [B, 13, 13, CO]
  const bf16* zero;   // >= 16 zero bytes
  int relu;
  // fused 3x3/s2 max-pool (AlexNet features.12 after features.10): [B, 6, 6, CO]
  // written instead of y (one pass per wave, ReLU on)
  bf16* ypool;
};
template <int CI_, int CO_, int PD_, int GPP_>
struct Direct13 {
  static constexpr int H = 13, W = 13, KS = 3, PAD = 1, CI = CI_, CO = CO_;
  static constexpr int WAVES = 4;  // one per SIMD
  static constexpr Split SPLIT = Split::Channels;
  // weight ring depth / 32-channel groups per pass: the largest without spills
  static constexpr int PD = PD_, GPP = GPP_;
  // one tile per wave, which needs the wave's channels in one pass (384 -> 256
  // has the form too, as in the kernels this file replaces, but only 256 -> 256
  // is offered: conv3x3_13_pool_supported)
  static constexpr Pool POOL = CO / 32 / WAVES == GPP ? Pool::PerWave : Pool::None;
  using Args = Args13;
  static constexpr bool RELU_ARG = true;
};

struct Direct27 {
  static constexpr int H = 27, W = 27, KS = 5, PAD = 2, CI = 64, CO = 192;
  static constexpr int WAVES = 8;  // 2 per SIMD
  static constexpr Split SPLIT = Split::Fragments;
  static constexpr int PD = 2, GPP = 2;
  static constexpr Pool POOL = Pool::PerGroup;  // one 32-channel group's tile, after the image
  struct Args {
    const bf16* x;      // [B, 27, 27, 64]
    const bf16* wf;     // [6][50][2][64][8] fragment order (stream_frag_index, K = 1600)
    const float* bias;  // [192]
    bf16* y;            // [B, 27, 27, 192]
    const bf16* zero;   // >= 16 zero bytes
    // fused 3x3/s2 max-pool (features.5): [B, 13, 13, 192] written instead of y
    bf16* ypool;
  };
  static constexpr bool RELU_ARG = false;
};

template <bool CH, int FPW> struct TapState { int pix[FPW], inm[FPW]; };
template <int FPW> struct TapState<true, FPW> {};

template <class S>
struct DirectGeom {
  static constexpr int NPIX = S::H * S::W;
  static constexpr int MFT = (NPIX + 15) / 16;                        // pixel fragments (the last partly padding)
  static constexpr int CPX = S::CI / 8;                               // 16-B chunks per pixel
  static constexpr int PXC = CPX > 8 ? (CPX + 15) / 16 * 16 : CPX;    // padded chunks per staged pixel
  static constexpr int PXB = PXC * 16;                                // bytes per staged pixel
  static constexpr int ZB = NPIX * PXB;                               // zero pixel
  static constexpr int XBYTES = ZB + PXB;                             // staged image + zero pixel
  static constexpr int CT = S::CI / 32;                               // K steps per tap
  static constexpr int KT = S::KS * S::KS * CT;                       // K steps
  static constexpr int NF = 2 * S::GPP;                               // N fragments per pass
  static constexpr bool CH = S::SPLIT == Split::Channels;
  static constexpr int FPW = CH ? MFT : (MFT + S::WAVES - 1) / S::WAVES;  // pixel fragments per wave
  static constexpr int NGW = CH ? S::CO / 32 / S::WAVES : S::CO / 32;     // 32-channel groups per wave
  static constexpr int PASSES = NGW / S::GPP;
  // fused pool: PH x PW pooled pixels; a tile pixel holds NC 16-B chunks
  // (PerWave: the wave's GPP groups; PerGroup: one group)
  static constexpr int PH = (S::H - 3) / 2 + 1, PW = (S::W - 3) / 2 + 1;
  static constexpr int NC = S::POOL == Pool::PerWave ? 4 * S::GPP : 4;
  static constexpr int TB = NC * 16;         // bytes per tile pixel
  static constexpr int TILE = NPIX * TB;     // bytes per tile
  // PerWave tiles overwrite the staged image, a PerGroup tile follows the zero pixel
  static constexpr int TILE0 = S::POOL == Pool::PerGroup ? XBYTES : 0;
  static constexpr size_t LDS = XBYTES;
  static constexpr size_t LDS_POOL = S::POOL == Pool::PerGroup ? (size_t)XBYTES + TILE : LDS;

  static_assert(CPX == 8 || CPX >= 16, "xswz covers 128-B pixels and pixels of >= 256 B");
  static_assert(PXC <= 64 * S::WAVES, "the zero pixel is written by one thread per chunk");
  static_assert(LDS_POOL <= 160 * 1024, "LDS budget");
  static_assert(NGW % S::GPP == 0, "passes");
  static_assert(CT % S::PD == 0, "the weight ring's slot must be a compile-time function of the K step in a tap");
  static_assert(!CH || S::CO % (32 * S::WAVES) == 0, "channel groups over the waves");
  static_assert(S::POOL != Pool::PerWave || (CH && PASSES == 1), "a wave's tile holds all its channels: one pass");
  // (at 256 -> 256 the four tiles are exactly the staged image's size)
  static_assert(S::POOL != Pool::PerWave || S::WAVES * TILE <= ZB, "the per-wave tiles overwrite the staged image");
  static_assert(S::POOL != Pool::PerGroup || TILE0 >= ZB + PXB, "the tile lies after the zero pixel");
};

template <class S>
__global__ __launch_bounds__(64 * S::WAVES, 1) void conv_direct_kernel(typename S::Args a) {
  using G = DirectGeom<S>;
  constexpr int H = S::H, W = S::W, KS = S::KS, PAD = S::PAD, CI = S::CI, CO = S::CO, PD = S::PD, GPP = S::GPP;
  constexpr int WAVES = S::WAVES, NPIX = G::NPIX, CPX = G::CPX, PXC = G::PXC, PXB = G::PXB, ZB = G::ZB;
  constexpr int CT = G::CT, KT = G::KT, NF = G::NF, FPW = G::FPW, NGW = G::NGW;
  constexpr bool CH = G::CH;
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  char* xs = (char*)smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, g = lane >> 4;
  const int b = blockIdx.x;
  const bf16* img = a.x + (long)b * NPIX * CI;

  // ---- stage the image: physical slot ps = K * PXC + pc holds logical chunk
  // pc ^ xswz(K) of pixel K (slots whose logical chunk is past CPX: padding,
  // loaded from the zero page); one LDS-DMA instruction = 64 slots
  constexpr int NSLOT = NPIX * PXC;
  for (int i = wave; i * 64 < NSLOT; i += WAVES) {
    const int ps = i * 64 + lane;
    if (ps < NSLOT) {
      // (each split's own spelling of one rule: the shared form, K = ps / PXC
      // with the `lc < CPX` test folded away, allocates registers differently)
      if constexpr (CH) {
        const int K = ps / PXC, pc = ps - K * PXC;
        const int lc = pc ^ xswz<CPX>(K);
        dma16(lc < CPX ? (const void*)(img + (long)K * CI + lc * 8) : (const void*)a.zero, xs + i * 1024);
      } else {
        const int K = ps >> 3, pc = ps & 7;
        dma16(img + (long)K * CI + (pc ^ xswz<CPX>(K)) * 8, xs + i * 1024);
      }
    }
  }
  // zero pixel (loop or single test: as the staging forms above)
  if constexpr (CH) {
    for (int i = tid; i < PXB / 16; i += 256) ((uint4*)(xs + ZB))[i] = make_uint4(0, 0, 0, 0);
  } else {
    if (tid < PXB / 16) ((uint4*)(xs + ZB))[tid] = make_uint4(0, 0, 0, 0);
  }

  // ---- per-lane pixel geometry: fragment f of this wave is pixels
  // p = 16 (f0 + f) + fr, clamped to the last pixel for padding lanes /
  // fragments (they compute a duplicate, never stored)
  const int f0 = CH ? 0 : wave * FPW;
  TapState<CH, FPW> ts;
  if constexpr (!CH) {
    // 27x27: pix[f] = the pixel's staged offset, inm[f] bit tap = the tap's
    // input pixel lies in the image. A tap then costs 3 VALU per fragment
    // (the 5x5 conv changes tap every 2 K steps: recomputing row / column per
    // tap was ~100 unhidden VALU per 48 MFMAs at one wave per SIMD).
#pragma unroll
    for (int f = 0; f < FPW; ++f) {
      const int p = min(16 * (f0 + f) + fr, NPIX - 1);
      const int r = W == 13 ? (p * 79) >> 10 : (p * 2428) >> 16, c = p - r * W;  // p / W, exact for p < NPIX
      int m = 0;
#pragma unroll
      for (int tap = 0; tap < KS * KS; ++tap) {
        const int kh = tap / KS, kw = tap % KS;
        if ((unsigned)(r + kh - PAD) < (unsigned)H && (unsigned)(c + kw - PAD) < (unsigned)W) m |= 1 << tap;
      }
      ts.pix[f] = p * PXB;
      ts.inm[f] = m;
    }
  }
  int xa[FPW], tsw = 0;
  auto set_tap = [&](int tap) __attribute__((always_inline)) {
    const int kh = tap / KS, kw = tap - kh * KS;
    const int ktap = (kh - PAD) * W + kw - PAD;
    if constexpr (CH) {
      // 13x13: row and column recomputed per tap (held across the K loop
      // they cost 11 VGPRs the loop needs)
#pragma unroll
      for (int f = 0; f < FPW; ++f) {
        const int p = min(16 * f + fr, NPIX - 1);
        const int r = W == 13 ? (p * 79) >> 10 : (p * 2428) >> 16, c = p - r * W;  // p / W, exact for p < NPIX
        const bool out = (kh == 0 && r == 0) || (kh == 2 && r == H - 1) || (kw == 0 && c == 0) ||
                         (kw == 2 && c == W - 1);
        xa[f] = out ? ZB : (p + ktap) * PXB;
      }
    } else {
      const int toff = ktap * PXB;
#pragma unroll
      for (int f = 0; f < FPW; ++f) xa[f] = ((ts.inm[f] >> tap) & 1) ? ts.pix[f] + toff : ZB;
    }
    // K = p + ktap with p & 15 == fr for every real pixel: one swizzle per tap
    tsw = (g << 4) ^ (xswz<CPX>(fr + ktap) << 4);
  };
  auto xread = [&](int f, int cc) __attribute__((always_inline)) {
    return *(const bf16x8*)(xs + xa[f] + (tsw ^ (cc * 64)));
  };
  vm_wait<0>();
  lds_barrier();

#pragma nounroll
  for (int pass = 0; pass < G::PASSES; ++pass) {
    const int grp0 = (CH ? wave * NGW : 0) + pass * GPP;  // first 32-channel group of this pass
    // this pass's groups grp0 .. grp0 + GPP - 1 are consecutive in the
    // fragment-order array; steps past the end re-load step 0 (uniform load
    // counts for the waits)
    // (compiler-visible buffer loads: untracked asm loads into a register
    // ring raced the register allocator at 254 VGPRs -- an in-flight load
    // landed in a reused register and faulted a later address)
    const __amdgpu_buffer_rsrc_t wrs =
        CH ? frag_rsrc(a.wf, grp0, GPP, KT) : wave_rsrc(a.wf + (long)grp0 * KT * 2 * 512, GPP * KT * 2 * 1024);
    auto wfetch = [&](int t, bf16x8* dst) __attribute__((always_inline)) {
      const int tt = t < KT ? t : 0;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) dst[nf] = frag_load(wrs, lane, KT, tt, nf);
    };
    bf16x8 wq[PD][NF];
#pragma unroll
    for (int t = 0; t < PD - 1; ++t) wfetch(t, wq[t]);
    floatx4 acc[FPW][NF];
#pragma unroll
    for (int f = 0; f < FPW; ++f)
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) acc[f][nf] = floatx4{0.f, 0.f, 0.f, 0.f};
    set_tap(0);
    bf16x8 xf[FPW];
#pragma unroll
    for (int f = 0; f < FPW; ++f) xf[f] = xread(f, 0);
#pragma nounroll
    for (int tap = 0; tap < KS * KS; ++tap) {
#pragma unroll
      for (int cc = 0; cc < CT; ++cc) {
        const int t = tap * CT + cc;
        wfetch(t + PD - 1, wq[(cc + PD - 1) % PD]);
        // next K step's X: same tap at cc + 1, or the next tap's first (the
        // final step re-reads a valid tile, unused)
        if (cc + 1 == CT && tap + 1 < KS * KS) set_tap(tap + 1);
        const int cn = cc + 1 == CT ? 0 : cc + 1;
        // the X fragments (read during the previous step) landed: one wait
        // instead of the compiler's one per fragment
        __builtin_amdgcn_s_waitcnt(0xC07F);
#pragma unroll
        for (int f = 0; f < FPW; ++f) {
#pragma unroll
          for (int nf = 0; nf < NF; ++nf)
            acc[f][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[cc % PD][nf], xf[f], acc[f][nf], 0, 0, 0);
          xf[f] = xread(f, cn);
        }
#pragma unroll
        for (int f = 0; f < FPW; ++f) {
          __builtin_amdgcn_sched_group_barrier(0x008, NF, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
      }
    }
    // ---- epilogue: lane holds channels 32 grp + 8 g .. +7 of pixel
    // 16 (f0 + f) + fr. The two pool forms keep the parent kernels' text: written
    // through shared tile-write / pool-maximum lambdas, the 13x13 kernels ran
    // 0.3-2.6 % slower (profiles/conv_direct.txt)
    if constexpr (S::POOL != Pool::None) {
      if (a.ypool) {
        // fused max-pool through an LDS tile [NPIX][NC chunks], chunk c of
        // pixel p at chunk c ^ (p & (NC - 1)); post-ReLU bf16 >= 0, so the
        // max is an unsigned 16-bit max
        typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));
        constexpr int NC = G::NC, TB = G::TB, PPIX = G::PH * G::PW;
        constexpr bool PW1 = S::POOL == Pool::PerWave;
        char* tile = xs + G::TILE0 + (PW1 ? wave * G::TILE : 0);
        if constexpr (PW1) {
          __syncthreads();
#pragma unroll
          for (int j = 0; j < GPP; ++j) {
            const int ch = 32 * (grp0 + j) + 8 * g;
            float bs[8];
            {
              const float4 lo = *(const float4*)(a.bias + ch), hi = *(const float4*)(a.bias + ch + 4);
              bs[0] = lo.x, bs[1] = lo.y, bs[2] = lo.z, bs[3] = lo.w, bs[4] = hi.x, bs[5] = hi.y, bs[6] = hi.z,
              bs[7] = hi.w;
            }
#pragma unroll
            for (int f = 0; f < FPW; ++f) {
              const int p = 16 * f + fr;
              if (p < NPIX) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = acc[f][2 * j + (e >> 2)][e & 3] + bs[e];
                *(uint4*)(tile + p * TB + (((4 * j + g) ^ (p & (4 * GPP - 1))) << 4)) = relu_bf16x8(pack8(v));
              }
            }
          }
          lgkm_wait();
          for (int it = lane; it < 36 * NC; it += 64) {
            const int pp = it / NC, c = it - pp * NC;
            const int ph = pp / 6, pw = pp - ph * 6;
            ushort8 m = ushort8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
              for (int dx = 0; dx < 3; ++dx) {
                const int q = (2 * ph + dy) * W + 2 * pw + dx;
                m = __builtin_elementwise_max(m, *(const ushort8*)(tile + q * TB + ((c ^ (q & (NC - 1))) << 4)));
              }
            *(ushort8*)(a.ypool + ((long)b * 36 + pp) * CO + 32 * grp0 + 8 * c) = m;
          }
        } else {
#pragma unroll
          for (int j = 0; j < GPP; ++j) {
            const int ch = 32 * (grp0 + j) + 8 * g;
            float bs[8];
            {
              const float4 lo = *(const float4*)(a.bias + ch), hi = *(const float4*)(a.bias + ch + 4);
              bs[0] = lo.x, bs[1] = lo.y, bs[2] = lo.z, bs[3] = lo.w, bs[4] = hi.x, bs[5] = hi.y, bs[6] = hi.z,
              bs[7] = hi.w;
            }
            __syncthreads();  // the previous group's pooling reads are done
#pragma unroll
            for (int f = 0; f < FPW; ++f) {
              const int p = 16 * (f0 + f) + fr;
              if (p < NPIX) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = acc[f][2 * j + (e >> 2)][e & 3] + bs[e];
                *(uint4*)(tile + p * 64 + ((g ^ (p & 3)) << 4)) = relu_bf16x8(pack8(v));
              }
            }
            __syncthreads();
            for (int it = threadIdx.x; it < 169 * 4; it += 64 * WAVES) {
              const int pp = it >> 2, c = it & 3;
              const int ph = (pp * 79) >> 10, pw = pp - ph * 13;  // pp / 13 for pp < 169
              ushort8 m = ushort8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
              for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                  const int q = (2 * ph + dy) * W + 2 * pw + dx;
                  m = __builtin_elementwise_max(m, *(const ushort8*)(tile + q * 64 + ((c ^ (q & 3)) << 4)));
                }
              *(ushort8*)(a.ypool + ((long)b * 169 + pp) * CO + 32 * (grp0 + j) + 8 * c) = m;
            }
          }
        }
        continue;
      }
    }
    bf16* yim = a.y + (long)b * NPIX * CO;
#pragma unroll
    for (int j = 0; j < GPP; ++j) {
      const int ch = 32 * (grp0 + j) + 8 * g;
      float bs[8];
      {
        const float4 lo = *(const float4*)(a.bias + ch), hi = *(const float4*)(a.bias + ch + 4);
        bs[0] = lo.x, bs[1] = lo.y, bs[2] = lo.z, bs[3] = lo.w, bs[4] = hi.x, bs[5] = hi.y, bs[6] = hi.z, bs[7] = hi.w;
      }
#pragma unroll
      for (int f = 0; f < FPW; ++f) {
        const int p = 16 * (f0 + f) + fr;
        if (p < NPIX) {
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = acc[f][2 * j + (e >> 2)][e & 3] + bs[e];
          if constexpr (S::RELU_ARG) *(uint4*)(yim + (long)p * CO + ch) = pack8_relu(v, a.relu);
          else *(uint4*)(yim + (long)p * CO + ch) = relu_bf16x8(pack8(v));
        }
      }
    }
  }
}

// Operands checked once for both entry points; then the launch.
template <class S>
void launch_direct(const char* name, const typename S::Args& a, int B, hipStream_t s) {
  using G = DirectGeom<S>;
  auto bad = [&](const char* what) { throw std::invalid_argument(std::string(name) + ": " + what); };
  // (with ypool given, y is not written and may be null)
  if (!a.x || !a.wf || !a.bias || !a.zero || (!a.y && !a.ypool)) bad("null operand");
  if (((uintptr_t)a.x | (uintptr_t)a.wf | (uintptr_t)a.bias | (uintptr_t)a.y | (uintptr_t)a.zero |
       (uintptr_t)a.ypool) & 15)
    bad("misaligned operand");
  // (no bound on B: the kernel indexes global memory in long and the ranges
  // below are sized in size_t, so no int B overflows either)
  // a workgroup stages its image while others already store theirs (only the
  // output that is written is checked: with ypool the kernel never writes y)
  const void* out = a.ypool ? a.ypool : a.y;
  if (ranges_overlap(a.x, (size_t)B * G::NPIX * S::CI * 2, out,
                     (size_t)B * (a.ypool ? G::PH * G::PW : G::NPIX) * S::CO * 2))
    bad("output overlaps the input");
  hipLaunchKernelGGL((conv_direct_kernel<S>), dim3(B), dim3(64 * S::WAVES), a.ypool ? G::LDS_POOL : G::LDS, s, a);
  DMLC_HIP_CHECK(hipGetLastError());
}

using D13a = Direct13<192, 384, 3, 1>;
using D13b = Direct13<384, 256, 3, 2>;
using D13c = Direct13<256, 256, 2, 2>;
static_assert(D13c::POOL == Pool::PerWave, "conv3x3_13_pool_supported names the 256 -> 256 shape");

}  // namespace

// the fused max-pool needs one pass per wave (the 256 -> 256 variant)
bool conv3x3_13_pool_supported(int Cin, int Cout) { return Cin == 256 && Cout == 256; }

bool conv3x3_13_supported(int H, int W, int Cin, int Cout) {
  return H == 13 && W == 13 &&
         ((Cin == 192 && Cout == 384) || (Cin == 384 && Cout == 256) || (Cin == 256 && Cout == 256));
}

bool conv5x5_27_supported(int H, int W, int Cin, int Cout, int pad) {
  return H == Direct27::H && W == Direct27::W && Cin == Direct27::CI && Cout == Direct27::CO && pad == Direct27::PAD;
}

void conv3x3_13(const void* x, const void* wf, const float* bias, void* y, const void* zero, int B, int Cin, int Cout,
                bool relu, hipStream_t s, void* ypool) {
  if (B <= 0) return;
  if (!conv3x3_13_supported(13, 13, Cin, Cout)) throw std::invalid_argument("conv3x3_13: unsupported channels");
  if (ypool && (!relu || !conv3x3_13_pool_supported(Cin, Cout)))
    throw std::invalid_argument("conv3x3_13: fused pool needs ReLU, Cin = Cout = 256");
  const Args13 a{(const bf16*)x, (const bf16*)wf, bias, (bf16*)y, (const bf16*)zero, relu ? 1 : 0, (bf16*)ypool};
  if (Cin == 192) launch_direct<D13a>("conv3x3_13", a, B, s);
  else if (Cin == 384) launch_direct<D13b>("conv3x3_13", a, B, s);
  else launch_direct<D13c>("conv3x3_13", a, B, s);
}

void conv5x5_27(const void* x, const void* wf, const float* bias, void* y, const void* zero, int B, hipStream_t s,
                void* ypool) {
  if (B <= 0) return;
  const Direct27::Args a{(const bf16*)x, (const bf16*)wf, bias, (bf16*)y, (const bf16*)zero, (bf16*)ypool};
  launch_direct<Direct27>("conv5x5_27", a, B, s);
}

}  // namespace dmlc
