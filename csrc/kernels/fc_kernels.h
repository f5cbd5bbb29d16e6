// Fully connected layers (AlexNet's classifier): y[M][N] = x[M][K] . W[N][K]^T,
// two designs, each a kernel template over the operand type. FP8 = false: bf16
// on v_mfma_f32_16x16x32_bf16. FP8 = true: e4m3 codes (OCP, one byte per
// element) on v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales (exact
// e4m3 x e4m3 products, fp32 accumulation): half the weight bytes, and the
// same operand bytes carry twice the K. fc.hip instantiates the bf16 forms,
// fc8.hip the e4m3 forms with their own compiler flags (tools/build.py).
//
// Reference equivalent: `classifier.{1,4,6}` (+ReLU) of tch::vision::alexnet,
// run per query by `forward_t` (src/services.rs:519-524, 493). The reference
// has no reduced-precision form.
//
// fc_small_kernel (B <= 16): weight-streaming GEMV on MFMA. The classifier
// (117 MB of bf16 weights) is pure weight bandwidth at query batch sizes: every
// weight is used B times. As an implicit-GEMM conv (conv_igemm.hip) the
// 128-row tiles leave 3/4 of the M dimension empty and ~16 workgroups stream
// the whole matrix; here the weight rows [Npad][ldw] as stored are the MFMA's A
// operand and the batch [B][ldx] is the B operand from the same byte positions
// (images in the 16 columns, zeros beyond B), so both operands agree on which
// K a byte stands for:
//
//  * one workgroup per 16 weight rows, its 8 waves split the K steps. In a
//    step lane (row = lane & 15, kq = lane >> 4) holds its row's 16 bytes
//    (8 bf16) or 32 bytes (32 e4m3, two 16-B loads) number kq; a wave keeps
//    16 KB of weight loads in flight (16 steps of 1 KB, or 8 of 2 KB). The
//    activations (a few hundred KB) stay L2-resident;
//  * the waves meet in LDS and one pass sums them in wave order, adds the
//    bias, applies ReLU and writes: a fixed summation order, no global
//    hand-off, no workspace. The two forms lay the partials out and finish
//    differently (below); their output bits are pinned by the suite.
//
// fc_gemm_kernel (M = B <= 256). On the implicit GEMM (128x128 tiles, 8 K
// slices) the three FCs took ~40 + ~20 + ~8 us plus three split-K reductions
// at B = 256, bound by the per-CU LDS-DMA ingest of the re-staged tiles
// (~30 GB/s per CU; profiles/r5_fc_splitk.txt). Here:
//
//  * a workgroup owns all M rows x 128 output columns x one K slice, so every
//    weight byte is read from HBM exactly once and the activations (<= 4.7 MB,
//    L2 / MALL resident) once per 128 columns;
//  * a stage is one K block of 128 bytes a row (64 bf16 or 128 e4m3: 32 KB of
//    activations + 16 KB of weights) brought to a 3-slot LDS ring by LDS-DMA,
//    two stages in flight while one is computed (with one in flight,
//    register-staged, the stages were load-latency bound at ~25 GB/s per CU),
//    16-B chunks XOR-swizzled by row through the source addresses;
//  * 8 waves = 2 row halves x 4 column quarters, 8 x 2 fragments. bf16: two
//    K steps of 32 a stage, a lane's operand is chunk 4 kk + fq of its row.
//    e4m3: ONE 16x16x128 MFMA per fragment pair and stage, a lane's operand is
//    chunks fq and fq + 4: the 16 lanes of a ds_read_b128 group (one fq, rows
//    fr = 0..15) then read physical chunks (fq ^ (fr & 7)) and that ^ 4, all
//    eight chunk columns twice over rows that are 128 B apart, conflict-free
//    exactly as the bf16 read is. Both operands read the same chunks, so which
//    K a byte stands for cancels in the sum;
//  * rows >= M read the zero page and are never stored. fp32 partials per K
//    slice go to the split-K workspace; each form reduces them its own way.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace dmlc {

namespace {

template <bool FP8>
using fc_elem = typename std::conditional<FP8, uint8_t, bf16>::type;
template <bool FP8>
using fc_frag = typename std::conditional<FP8, v8i, bf16x8>::type;  // a lane's MFMA operand

template <bool FP8>
__device__ __forceinline__ floatx4 fc_mfma(fc_frag<FP8> a, fc_frag<FP8> b, floatx4 c) {
  if constexpr (FP8) return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------- fc_small
constexpr int kWaves = 8;  // waves per workgroup = K split of one 16-row tile

struct FcSmallArgs {
  const bf16* x;      // [B, K] (row stride ldx)
  const bf16* w;      // [Npad, ldw]
  const float* bias;  // [Npad]
  void* y;            // [B, ldo] bf16 or fp32
  int B, K, N, ldx, ldw, ldo;
  int relu, out_f32;
};

struct FcSmall8Args {
  const uint8_t* x;    // [B, ldx] e4m3
  const uint8_t* w;    // [Npad, ldw] e4m3
  const float* alpha;  // [Npad]
  const float* bias;   // [Npad]
  void* y;             // [B, ldo]
  int B, K, N, ldx, ldw, ldo;
  int relu, out_kind;
  float out_inv_scale;
};

// The e4m3 form's finish (fc8.hip): t as the output kind's bits at element o of y.
__device__ __forceinline__ void store_out(void* y, long o, float t, int kind, float out_inv_scale);

template <bool FP8>
__global__ __launch_bounds__(64 * kWaves) void fc_small_kernel(
    typename std::conditional<FP8, FcSmall8Args, FcSmallArgs>::type a) {
  constexpr int KS = FP8 ? 128 : 32;  // K per step (one MFMA)
  constexpr int LE = KS / 4;          // a lane's elements of a step
  constexpr int U = FP8 ? 8 : 16;     // steps with their weight loads in flight per wave (16 KB)
  __shared__ __attribute__((aligned(16))) float part[kWaves][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const int row = lane & 15, kq = lane >> 4;  // A: weight row n0 + row, elements LE kq ..; B: image col = row
  const int ksteps = a.K / KS, per = (ksteps + kWaves - 1) / kWaves;
  // (the two forms bound ks0 and form a masked step's address each in its own
  // way below: either is correct for both, and each keeps its instructions)
  const int ks0 = FP8 ? min(wave * per, ksteps) : wave * per, ks1 = min(ks0 + per, ksteps);
  const fc_elem<FP8>* wrow = a.w + (long)(n0 + row) * a.ldw + kq * LE;
  const bool live = row < a.B;
  const fc_elem<FP8>* xrow = a.x + (long)(live ? row : 0) * a.ldx + kq * LE;
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int ks = ks0; ks < ks1; ks += U) {
    fc_frag<FP8> wv[U], xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in = ks + u < ks1;
      if constexpr (FP8) {
        const long k = (long)(in ? ks + u : ks) * KS;  // (a step past the range repeats a valid address, unused)
        wv[u] = in ? e4m3x32(*(const uint4*)(wrow + k), *(const uint4*)(wrow + k + 16)) : v8i{};
        xv[u] = (in && live) ? e4m3x32(*(const uint4*)(xrow + k), *(const uint4*)(xrow + k + 16)) : v8i{};
      } else {
        const int k = (ks + u) * KS;
        wv[u] = in ? *(const bf16x8*)(wrow + k) : bf16x8{};
        xv[u] = (in && live) ? *(const bf16x8*)(xrow + k) : bf16x8{};
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc = fc_mfma<FP8>(wv[u], xv[u], acc);
  }
  // lane holds D[rows 4 kq .. 4 kq + 3][col = row]. Thread tid < 256 finishes
  // the element whose 8 partials sit at part[.][tid]: bf16 keeps element
  // (r, c) at 16 r + c (scalar stores), e4m3 at 16 c + r (one 16-B store)
  if constexpr (FP8) {
    *(floatx4*)&part[wave][row * 16 + 4 * kq] = acc;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][(4 * kq + r) * 16 + row] = acc[r];
  }
  __syncthreads();
  if (tid >= 256) return;
  const int r = FP8 ? tid & 15 : tid >> 4, c = FP8 ? tid >> 4 : tid & 15, n = n0 + r;
  if (c >= a.B || n >= a.N) return;
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) t += part[w][tid];
  if constexpr (FP8) t = __builtin_fmaf(t, a.alpha[n], a.bias[n]);
  else t += a.bias[n];
  if (a.relu) t = fmaxf(t, 0.f);
  if constexpr (FP8) store_out(a.y, (long)c * a.ldo + n, t, a.out_kind, a.out_inv_scale);
  else if (a.out_f32) ((float*)a.y)[(long)c * a.ldo + n] = t;
  else ((bf16*)a.y)[(long)c * a.ldo + n] = f2bf(t);
}

// ---------------------------------------------------------------- fc_gemm
constexpr int kBM = 256;          // rows (images) per workgroup: all of them
constexpr int kBN = 128;          // output columns per workgroup
constexpr int kAB = kBM * 128;    // 32 KB A stage: a K block is 128 bytes a row
constexpr int kBB = kBN * 128;    // 16 KB B stage
constexpr int kStage = kAB + kBB;
static_assert(kAB / 1024 == 32 && kBB / 1024 == 16, "6 DMA instructions per wave per stage");
static_assert(3 * kStage <= 160 * 1024, "LDS per CU");
template <bool FP8>
constexpr int kFcKB = FP8 ? 128 : 64;  // K block per stage (elements)

template <bool FP8>
__global__ __launch_bounds__(512, 1) void fc_gemm_kernel(const fc_elem<FP8>* __restrict__ x,
                                                         const fc_elem<FP8>* __restrict__ w, float* __restrict__ ws,
                                                         int M, int K, int Npad, int kslice, int nslices,
                                                         const fc_elem<FP8>* __restrict__ zero) {
  constexpr int KB = kFcKB<FP8>;
  constexpr int CE = KB / 8;  // elements per 16-B chunk
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  char* lds = (char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int fr = lane & 15, fq = lane >> 4;
  // workgroup -> (column block nb, K slice ks). Workgroups are dealt to the 8
  // XCDs round-robin: with a multiple of 8 slices, XCD x takes slices x, x+8,
  // ... for every column block, so each XCD's L2 holds only its own slices'
  // activations (read once from HBM chip-wide) instead of all of them
  const int cols = Npad / kBN, L = blockIdx.x;
  int nb, ks;
  if (nslices % 8 == 0) {
    const int i = L >> 3;
    nb = i % cols;
    ks = (L & 7) + 8 * (i / cols);
  } else {
    nb = L % cols;
    ks = L / cols;
  }
  const int n0 = nb * kBN;
  const int k0 = ks * kslice;
  const int nstages = kslice / KB;

  // Staging: a 3-slot LDS ring filled by LDS-DMA (global_load_lds_dwordx4,
  // 1 KB per wave instruction: lane l's 16 B land at slot offset 1024 i +
  // 16 l), two K blocks in flight while one is computed. A stage is 32 A
  // instructions (256 rows x 128 B) + 16 B instructions (128 rows), 6 per
  // wave; LDS position p = 64 i + l holds row p >> 3, physical chunk p & 7 =
  // logical chunk (p & 7) ^ (row & 7), so the source address carries the
  // swizzle. Rows >= M read the zero page.
  floatx4 acc[8][2];
#pragma unroll
  for (int mf = 0; mf < 8; ++mf)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) acc[mf][nf] = floatx4{0.f, 0.f, 0.f, 0.f};
  const fc_elem<FP8>* asrc[4];
  const fc_elem<FP8>* bsrc[2];
  int aoff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = (4 * wave + j) * 64 + lane, r = p >> 3, lc = (p & 7) ^ (r & 7);
    asrc[j] = r < M ? x + (long)r * K + k0 + CE * lc : zero;
    aoff[j] = r < M ? 1 : 0;  // (the zero page does not advance with K)
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = (2 * wave + j) * 64 + lane, r = p >> 3, lc = (p & 7) ^ (r & 7);
    bsrc[j] = w + (long)(n0 + r) * K + k0 + CE * lc;
  }
  auto dma_stage = [&](int st, int slot) __attribute__((always_inline)) {
    char* base = lds + slot * kStage;
    const int ko = st * KB;
#pragma unroll
    for (int j = 0; j < 4; ++j) dma16(asrc[j] + ko * aoff[j], base + (4 * wave + j) * 1024);
#pragma unroll
    for (int j = 0; j < 2; ++j) dma16(bsrc[j] + ko, base + kAB + (2 * wave + j) * 1024);
  };
  // a lane's operand of row `row` in MFMA step kk of the stage
  auto frag = [&](const char* region, int row, int kk) __attribute__((always_inline)) {
    if constexpr (FP8)
      return e4m3x32(*(const uint4*)(region + swz128(row, fq)), *(const uint4*)(region + swz128(row, fq + 4)));
    else return *(const bf16x8*)(region + swz128(row, 4 * kk + fq));
  };
  dma_stage(0, 0);
  if (nstages > 1) dma_stage(1, 1);
  for (int s = 0; s < nstages; ++s) {
    // this wave's DMA of stage s has landed (stage s+1's may stay in flight),
    // and after the barrier everyone's has, and every wave is done with stage
    // s-1, whose slot stage s+2 reuses
    if (s + 1 < nstages) vm_wait<6>();
    else vm_wait<0>();
    __builtin_amdgcn_s_barrier();
    if (s + 2 < nstages) dma_stage(s + 2, (s + 2) % 3);
    const char* base = lds + (s % 3) * kStage;
#pragma unroll
    for (int kk = 0; kk < (FP8 ? 1 : 2); ++kk) {
      fc_frag<FP8> af[8], bf[2];
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) af[mf] = frag(base, 128 * wm + 16 * mf + fr, kk);
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) bf[nf] = frag(base + kAB, 32 * wn + 16 * nf + fr, kk);
#pragma unroll
      for (int mf = 0; mf < 8; ++mf)
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) acc[mf][nf] = fc_mfma<FP8>(af[mf], bf[nf], acc[mf][nf]);
    }
    lgkm_wait();  // (this wave's reads of the slot are done)
  }
  // D lane (fr, fq): row 4 fq + r of the fragment, column fr
  float* wsp = ws + (long)ks * M * Npad;
#pragma unroll
  for (int mf = 0; mf < 8; ++mf)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      const int n = n0 + 32 * wn + 16 * nf + fr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 128 * wm + 16 * mf + 4 * fq + r;
        if (m < M) wsp[(long)m * Npad + n] = acc[mf][nf][r];
      }
    }
}

// K slices: about one workgroup per CU, each at least 4 K blocks
template <bool FP8>
int fc_gemm_splits_rule(const ConvArgs& a, int num_cus) {
  if (a.Kpad <= 0 || a.Npad <= 0 || a.Npad % kBN) return 0;
  const int kb = a.Kpad / kFcKB<FP8>;
  const int cols = a.Npad / kBN;
  int s = std::max(1, std::min(kb / 4, (num_cus + cols - 1) / cols));
  while (s > 1 && kb % s) --s;  // whole K blocks per slice
  return s;
}

// The partials of a layer its form's *_supported accepts, into a.ws [splits][M][Npad].
template <bool FP8>
void fc_gemm_launch(const ConvArgs& a, int splits, hipStream_t s) {
  hipLaunchKernelGGL(fc_gemm_kernel<FP8>, dim3(a.Npad / kBN * splits), dim3(512), (size_t)3 * kStage, s,
                     (const fc_elem<FP8>*)a.x, (const fc_elem<FP8>*)a.w, a.ws, a.B, a.Kpad, a.Npad, a.Kpad / splits,
                     splits, (const fc_elem<FP8>*)a.zero);
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace

}  // namespace dmlc
