// Query-batch 1x1 conv (B <= a few images), stride 1 or 2, no padding, NHWC,
// bf16 or e4m3 in (v_mfma_f32_16x16x32_bf16 / the block-scaled
// v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales), bf16 or e4m3 out
// whatever the input type: ResNet50's bottleneck reduce / expand convs and its
// 1x1/s2 downsamples at the serving fleet's batch-1 query shape.
//
// Reference equivalent: Bottleneck.conv1 / conv3 / downsample.0 of
// tch::vision::resnet50, run for ONE image per query by `forward_t`. At B = 1
// a 1x1 conv is a skinny GEMM (M = 49..3136 pixels, K up to 2048): conv1x1.hip
// walks 64-pixel blocks weight-stationary (1-49 workgroups), the implicit GEMM
// has 128x128 / 64x256 tiles with a split-K pass and a splitk_reduce launch
// behind it (bf16) or no split-K at all (e4m3), and bottleneck56.hip runs a
// whole 56x56 bottleneck on one CU. Here, as in fc_small / conv_small /
// conv_small8, the cost is one dependent memory round trip:
//
//  * the pixel axis is flat over the batch, M = B Ho Wo, 16 pixels a fragment
//    (stride 1: fragments may straddle images; stride 2: pixel p of image b
//    reads x[b, 2 oy, 2 ox] by address arithmetic). A workgroup owns NF
//    16-channel fragments x MF pixel fragments: grid = (N / 16 / NF,
//    ceil(M / 16 / MF)). conv1x1_small_pick takes the largest tile that still
//    gives about one workgroup per CU (total operand traffic goes with 1 / MF +
//    1 / NF), else the tile with the most workgroups: at B = 1 the grid is what
//    puts CUs to work (conv_small8.hip's header has the argument);
//  * the weights are the A operand, read from the layer's row-major [Npad][Kpad]
//    rows as they are: lane (fr, g) takes 16 B (bf16: k = 32 s + 8 g .. + 8) or
//    2 x 16 B (e4m3: bytes 128 s + 32 g .. + 32) of channel row 16 nf + fr, and
//    the same bytes of its pixel's channel row for B, so which k a byte stands
//    for cancels. A lane ends with channels 16 nf + 4 g .. + 3 of pixel fr:
//    8-B bf16 / 4-B e4m3 residual loads and stores;
//  * the 4 waves are WK along K x WM = 4 / WK along the tile's pixel fragments
//    (wave = wm WK + wk; its fragments f = wm, wm + WM, ..). WK = 4 where that
//    leaves a wave at least one K step (bf16 K >= 128, e4m3 K >= 512), WK = 2
//    for e4m3 K = 256, WK = 1 for bf16 K = 64 and e4m3 K = 128 (the waves split
//    the pixel fragments and nothing is reduced). A wave's KSW K steps are one
//    contiguous K range, so a row's cache lines are read whole by one wave;
//  * a 1x1 conv reads each input element once per channel tile: there is no
//    tap reuse to stage for, so both operands go straight from L2 into
//    registers in fragment layout, and every global load of the wave (KSW x
//    (NF + MFW) fragments, step by step) is issued before its first MFMA: one
//    memory round trip, the MFMAs of step s starting when its operands land
//    (the compiler's counted vmcnt waits). fits() bounds KSW (MFW + NF) x 4 or 8
//    operand VGPRs at 256;
//  * rows past M read pixel 0 and are not stored;
//  * WK > 1: the waves' fp32 partial sums meet in LDS ([wk][f][nf][lane]) and
//    are added in wave order 0 .. WK-1, so the bits do not depend on timing;
//    wave t then finishes fragment t, t + 4, .. of the tile's MF x NF;
//  * epilogue (conv1x1.hip's arithmetic, one fma a value): q = fma(acc, alpha[n]
//    osc, bias[n] osc) (alpha = 1 for bf16 in, osc = out_inv_scale for e4m3 out,
//    else 1), residual of the output's type (bf16: q += r; e4m3: q = fma(r,
//    res_scale osc, q)), then bf16(relu(q)) or e4m3(med3(q, relu ? 0 : -448,
//    448)).
//
// VGPRs over a form's tiles, (1,1) .. the largest tile fits() admits (hipcc
// -Rpass-analysis=kernel-resource-usage; the bf16 forms keep their accumulators
// in up to 192 AGPRs besides; no scratch in any of the 58 instantiations):
//   bf16 WK x KSW = 1x2 (K = 64)    28 ..  78     e4m3 1x1 (K = 128)   32 .. 108
//   bf16 4x1 (K = 128)              22 ..  82     e4m3 2x1 (K = 256)   32 ..  86
//   bf16 4x2 (K = 256)              30 .. 114     e4m3 4x1 (K = 512)   34 .. 118
//   bf16 4x4 (K = 512)              46 .. 200     e4m3 4x2 (K = 1024)  50 .. 208
//   bf16 4x8 (K = 1024)             76 .. 200     e4m3 4x4 (K = 2048)  78 .. 206
//   bf16 4x16 (K = 2048)           140 .. 200
//
// Compiled without packed fp32 VALU ops (tools/build.py).
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <type_traits>

namespace dmlc {

namespace {

struct S1Args {
  const uint8_t* x;    // [B, H, W, Cin] bf16 or e4m3
  const uint8_t* w;    // [Npad][Kpad] bf16 or e4m3
  const float* alpha;  // [N] (e4m3 in)
  const float* bias;   // [N]
  const uint8_t* res;  // [M, N] of the output's type, or null
  uint8_t* y;          // [M, N] bf16 or e4m3
  int M, HoWo, Wo, H, W, N, stride;
  int xrow, wrow;      // bytes of a pixel's / a weight row's channels
  int out8, relu;
  float osc, rsc;      // e4m3 out: out_inv_scale and res_scale * out_inv_scale; else 1, 1
};

// operand VGPRs of a wave: KSW K steps x (its pixel fragments + NF) x 4 (bf16) / 8 (e4m3)
constexpr bool fits(bool in8, int wk, int ksw, int mf, int nf) {
  const int wm = 4 / wk, mfw = (mf + wm - 1) / wm;
  return ksw * (mfw + nf) * (in8 ? 8 : 4) <= 256;
}

template <bool IN8, int WK, int KSW, int MF, int NF>
__global__ __launch_bounds__(256, 1) void conv1x1_small_kernel(S1Args a) {
  constexpr int WM = 4 / WK;
  constexpr int MFW = (MF + WM - 1) / WM;  // pixel fragments per wave
  constexpr int SB = IN8 ? 128 : 64;       // bytes of a channel row per K step
  using Frag = typename std::conditional<IN8, v8i, bf16x8>::type;
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  floatx4* part = (floatx4*)smem;  // WK > 1: [wk][f][nf][lane]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wave % WK, wm = wave / WK;
  const int fr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (NF * 16);
  const int f0 = blockIdx.y * MF;
  const int koff = wk * KSW * SB + g * (SB / 4);  // this lane's bytes of K step 0 of the wave's range

  const uint8_t* wp[NF];
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) wp[nf] = a.w + (long)(n0 + 16 * nf + fr) * a.wrow + koff;
  const uint8_t* xp[MFW];
#pragma unroll
  for (int j = 0; j < MFW; ++j) {
    const int f = wm + WM * j;
    int p = (f0 + f) * 16 + fr;
    if (f >= MF || p >= a.M) p = 0;  // a valid address, never stored
    long pix = p;
    if (a.stride == 2) {
      const int b = p / a.HoWo, r = p - b * a.HoWo;
      const int oy = r / a.Wo, ox = r - oy * a.Wo;
      pix = ((long)b * a.H + 2 * oy) * a.W + 2 * ox;
    }
    xp[j] = a.x + pix * a.xrow + koff;
  }

  // ---- the epilogue's constants first (they land first): the channels this
  // wave finishes are nf = 0 .. NF-1 of its own fragments (WK = 1), or the one
  // nf = (wave + 4 i) % NF = wave % NF of the fragments it reduces
  constexpr int EN = WK == 1 ? NF : 1;
  float al[EN][4], bs[EN][4];
#pragma unroll
  for (int e = 0; e < EN; ++e) {
    const int ch = n0 + 16 * (WK == 1 ? e : wave % NF) + 4 * g;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      al[e][i] = (IN8 ? a.alpha[ch + i] : 1.f) * a.osc;
      bs[e][i] = a.bias[ch + i] * a.osc;
    }
  }

  // ---- every operand load of the wave, K step by K step
  auto ld = [](const uint8_t* p) __attribute__((always_inline)) {
    if constexpr (IN8) return e4m3x32(*(const uint4*)p, *(const uint4*)(p + 16));
    else return *(const bf16x8*)p;
  };
  Frag wr[KSW][NF], xr[KSW][MFW];
#pragma unroll
  for (int s = 0; s < KSW; ++s) {
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) wr[s][nf] = ld(wp[nf] + s * SB);
#pragma unroll
    for (int j = 0; j < MFW; ++j) xr[s][j] = ld(xp[j] + s * SB);
  }
  // (the scheduler would otherwise sink loads between the MFMAs to save
  // registers: a dependent round trip per step instead of one per kernel)
  __builtin_amdgcn_sched_barrier(0);

  floatx4 acc[MFW][NF];
#pragma unroll
  for (int j = 0; j < MFW; ++j)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[j][nf] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < KSW; ++s)
#pragma unroll
    for (int j = 0; j < MFW; ++j)
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        if constexpr (IN8)
          acc[j][nf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wr[s][nf], xr[s][j], acc[j][nf], 0, 0, 0, 127,
                                                                         0, 127);
        else
          acc[j][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[s][nf], xr[s][j], acc[j][nf], 0, 0, 0);
      }

  // ---- epilogue of pixel fragment f x channel fragment nf: the lane's 4 channels of pixel fr
  const float lo_clamp = a.relu ? 0.f : -448.f;
  auto finish = [&](floatx4 v, int f, int nf, int e) __attribute__((always_inline)) {
    const int p = (f0 + f) * 16 + fr;
    if (p >= a.M) return;
    const int ch = n0 + 16 * nf + 4 * g;
    const long o = (long)p * a.N + ch;
    float q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = __builtin_fmaf(v[i], al[e][i], bs[e][i]);
    if (a.out8) {
      if (a.res) {
        float rv[4];
        e4m3x4_to_f32(*(const uint32_t*)(a.res + o), rv);
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = __builtin_fmaf(rv[i], a.rsc, q[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = __builtin_amdgcn_fmed3f(q[i], lo_clamp, 448.f);
      *(uint32_t*)(a.y + o) = e4m3x4_from_f32(q[0], q[1], q[2], q[3]);
    } else {
      if (a.res) {
        const uint2 r = *(const uint2*)(a.res + 2 * o);
        q[0] += __uint_as_float(r.x << 16);
        q[1] += __uint_as_float(r.x & 0xffff0000u);
        q[2] += __uint_as_float(r.y << 16);
        q[3] += __uint_as_float(r.y & 0xffff0000u);
      }
      if (a.relu) {
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = __builtin_amdgcn_fmed3f(q[i], 0.f, __builtin_inff());
      }
      *(uint2*)(a.y + 2 * o) = make_uint2(pack2(q[0], q[1]), pack2(q[2], q[3]));
    }
  };

  if constexpr (WK == 1) {
#pragma unroll
    for (int j = 0; j < MFW; ++j) {
      const int f = wm + WM * j;
      if (f >= MF) break;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) finish(acc[j][nf], f, nf, nf);
    }
  } else {
#pragma unroll
    for (int j = 0; j < MFW; ++j) {
      const int f = wm + WM * j;
      if (f >= MF) break;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) part[((wk * MF + f) * NF + nf) * 64 + lane] = acc[j][nf];
    }
    __syncthreads();
    for (int t = wave; t < MF * NF; t += 4) {
      floatx4 v = part[t * 64 + lane];
#pragma unroll
      for (int k = 1; k < WK; ++k) v += part[(k * MF * NF + t) * 64 + lane];
      finish(v, t / NF, t % NF, 0);
    }
  }
}

// (waves along K, K steps per wave) of a K, or wk = 0
struct Form {
  int wk = 0, ksw = 0;
};
Form form_of(bool in8, int cin) {
  Form f;
  const int step = in8 ? 128 : 32;
  if (cin <= 0 || cin % step) return f;
  const int steps = cin / step;
  const int wk = in8 ? (steps >= 4 ? 4 : steps) : (steps >= 4 ? 4 : 1);
  const int ksw = steps / wk;
  // the instantiated forms: bf16 K = 64, 128 .. 2048; e4m3 K = 128, 256, 512 .. 2048
  const bool have = in8 ? ((wk < 4 && ksw == 1) || (wk == 4 && (ksw == 1 || ksw == 2 || ksw == 4)))
                        : ((wk == 1 && ksw == 2) || (wk == 4 && (ksw & (ksw - 1)) == 0 && ksw <= 16));
  if (!have || steps != wk * ksw) return f;
  f.wk = wk;
  f.ksw = ksw;
  return f;
}

// the (MF, NF) tiles, largest first
constexpr int kTiles[6][2] = {{8, 4}, {8, 2}, {4, 2}, {4, 1}, {2, 1}, {1, 1}};

bool tile_ok(const ConvArgs& a, const Form& fm, int mf, int nf) {
  for (const auto& t : kTiles)
    if (t[0] == mf && t[1] == nf) return fits(a.in_fp8, fm.wk, fm.ksw, mf, nf) && (a.N / 16) % nf == 0;
  return false;
}

template <bool IN8, int WK, int KSW, int MF, int NF>
bool try_launch(const S1Args& s, int mf, int nf, hipStream_t st) {
  if constexpr (fits(IN8, WK, KSW, MF, NF)) {
    if (mf == MF && nf == NF) {
      const dim3 grid(s.N / (16 * NF), (s.M + 16 * MF - 1) / (16 * MF));
      const size_t lds = WK > 1 ? (size_t)WK * MF * NF * 64 * 16 : 0;
      hipLaunchKernelGGL((conv1x1_small_kernel<IN8, WK, KSW, MF, NF>), grid, dim3(256), lds, st, s);
      return true;
    }
  }
  return false;
}

template <bool IN8, int WK, int KSW>
bool launch_tile(const S1Args& s, int mf, int nf, hipStream_t st) {
  return try_launch<IN8, WK, KSW, 8, 4>(s, mf, nf, st) || try_launch<IN8, WK, KSW, 8, 2>(s, mf, nf, st) ||
         try_launch<IN8, WK, KSW, 4, 2>(s, mf, nf, st) || try_launch<IN8, WK, KSW, 4, 1>(s, mf, nf, st) ||
         try_launch<IN8, WK, KSW, 2, 1>(s, mf, nf, st) || try_launch<IN8, WK, KSW, 1, 1>(s, mf, nf, st);
}

bool launch_form(bool in8, const Form& fm, const S1Args& s, int mf, int nf, hipStream_t st) {
  const int key = (in8 ? 1000 : 0) + fm.wk * 100 + fm.ksw;
  switch (key) {
    case 102: return launch_tile<false, 1, 2>(s, mf, nf, st);
    case 401: return launch_tile<false, 4, 1>(s, mf, nf, st);
    case 402: return launch_tile<false, 4, 2>(s, mf, nf, st);
    case 404: return launch_tile<false, 4, 4>(s, mf, nf, st);
    case 408: return launch_tile<false, 4, 8>(s, mf, nf, st);
    case 416: return launch_tile<false, 4, 16>(s, mf, nf, st);
    case 1101: return launch_tile<true, 1, 1>(s, mf, nf, st);
    case 1201: return launch_tile<true, 2, 1>(s, mf, nf, st);
    case 1401: return launch_tile<true, 4, 1>(s, mf, nf, st);
    case 1402: return launch_tile<true, 4, 2>(s, mf, nf, st);
    case 1404: return launch_tile<true, 4, 4>(s, mf, nf, st);
    default: return false;
  }
}

}  // namespace

bool conv1x1_small_supported(const ConvArgs& a) {
  if (a.KH != 1 || a.KW != 1 || a.pad != 0 || (a.stride != 1 && a.stride != 2)) return false;
  if (a.x2 || a.split_k > 1 || a.out_f32 || a.stem) return false;
  if (a.B <= 0 || a.H <= 0 || a.W <= 0 || a.N <= 0 || a.N % 16 || a.ldo != a.N || a.Kpad < a.Cin) return false;
  if (a.Ho != conv_out_dim(a.H, 1, a.stride, 0) || a.Wo != conv_out_dim(a.W, 1, a.stride, 0)) return false;
  if ((a.Kpad * (a.in_fp8 ? 1 : 2)) % 16) return false;
  const long M = (long)a.B * a.Ho * a.Wo;
  if ((long)a.B * a.H * a.W * a.Cin >= (1L << 30) || M * a.N >= (1L << 30)) return false;  // 32-bit pixel indices
  return form_of(a.in_fp8, a.Cin).wk > 0;
}

std::pair<int, int> conv1x1_small_pick(const ConvArgs& a, int num_cus) {
  if (!conv1x1_small_supported(a)) throw std::invalid_argument("conv1x1_small_pick: unsupported shape");
  const Form fm = form_of(a.in_fp8, a.Cin);
  const long frags = ((long)a.B * a.Ho * a.Wo + 15) / 16;
  std::pair<int, int> best{1, 1};
  long best_wgs = 0;
  for (const auto& t : kTiles) {
    if (!tile_ok(a, fm, t[0], t[1])) continue;
    const long wgs = (a.N / 16 / t[1]) * ((frags + t[0] - 1) / t[0]);
    // the largest tile with about one workgroup per CU, else the most workgroups
    if (4 * wgs >= 3L * num_cus) return {t[0], t[1]};
    if (wgs > best_wgs) {
      best_wgs = wgs;
      best = {t[0], t[1]};
    }
  }
  return best;
}

void conv1x1_small(const ConvArgs& a, int mf, int nf, hipStream_t s) {
  if (!conv1x1_small_supported(a)) throw std::invalid_argument("conv1x1_small: unsupported shape");
  const Form fm = form_of(a.in_fp8, a.Cin);
  if (!tile_ok(a, fm, mf, nf)) throw std::invalid_argument("conv1x1_small: no such (mf, nf) tile for this shape");
  if (!a.x || !a.w || !a.bias || !a.y || (a.in_fp8 && !a.alpha))
    throw std::invalid_argument("conv1x1_small: null operand");
  const size_t oa = a.out_fp8 ? 3 : 7;  // a lane's 4 channels: 4 B e4m3, 8 B bf16
  if ((((uintptr_t)a.x | (uintptr_t)a.w) & 15) || (((uintptr_t)a.y | (uintptr_t)a.res) & oa) ||
      (((uintptr_t)a.bias | (uintptr_t)a.alpha) & 3))
    throw std::invalid_argument("conv1x1_small: misaligned operand");
  if (a.out_fp8 && !(a.out_inv_scale > 0.f)) throw std::invalid_argument("conv1x1_small: no output scale");
  const long M = (long)a.B * a.Ho * a.Wo;
  const size_t xn = (size_t)a.B * a.H * a.W * a.Cin * (a.in_fp8 ? 1 : 2), yn = (size_t)M * a.N * (a.out_fp8 ? 1 : 2);
  if (ranges_overlap(a.x, xn, a.y, yn)) throw std::invalid_argument("conv1x1_small: in-place not supported");
  if (a.res && ranges_overlap(a.res, yn, a.y, yn)) throw std::invalid_argument("conv1x1_small: res overlaps y");
  if ((M + 16 * mf - 1) / (16 * mf) > 65535) throw std::invalid_argument("conv1x1_small: batch too large");
  S1Args k;
  k.x = (const uint8_t*)a.x;
  k.w = (const uint8_t*)a.w;
  k.alpha = a.alpha;
  k.bias = a.bias;
  k.res = (const uint8_t*)a.res;
  k.y = (uint8_t*)a.y;
  k.M = (int)M;
  k.HoWo = a.Ho * a.Wo;
  k.Wo = a.Wo;
  k.H = a.H;
  k.W = a.W;
  k.N = a.N;
  k.stride = a.stride;
  k.xrow = a.Cin * (a.in_fp8 ? 1 : 2);
  k.wrow = a.Kpad * (a.in_fp8 ? 1 : 2);
  k.out8 = a.out_fp8;
  k.relu = a.relu;
  k.osc = a.out_fp8 ? a.out_inv_scale : 1.f;
  k.rsc = a.out_fp8 ? a.res_scale * a.out_inv_scale : 1.f;
  if (!launch_form(a.in_fp8, fm, k, mf, nf, s)) throw std::logic_error("conv1x1_small: no kernel for the picked tile");
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
