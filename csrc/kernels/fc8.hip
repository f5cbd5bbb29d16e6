// Fully connected layers on e4m3 (OCP, one byte per weight): AlexNet's
// classifier.1 / classifier.4 of the `alexnet_fp8` arch.
//
// Reference equivalent: `classifier.{1,4}` (+ReLU) of tch::vision::alexnet,
// run per query by `forward_t` (src/services.rs:519-524, 493). The reference
// has no reduced-precision form; this is fc_small.hip / fc_gemm.hip with half
// the weight bytes, on v_mfma_scale_f32_16x16x128_f8f6f4 with unit block
// scales (exact e4m3 x e4m3 products, fp32 accumulation).
//
// y[b][n] = act((sum_k cx[b][k] cw[n][k]) alpha[n] + bias[n]), cx / cw the
// e4m3 codes, alpha[n] = s_x s_w[n] (the activation's per-tensor scale times
// the weight row's), written as bf16, fp32 or e4m3(y out_inv_scale)
// (saturating, common.h's clamped converter).
//
// quant_e4m3_kernel: bf16 rows -> e4m3(v inv_scale). A thread owns 8 values:
// one 16-B load, one 8-B store.
//
// fc_small8_kernel (B <= 16): fc_small.hip's split. One workgroup per 16
// weight rows, its 8 waves split the K / 128 steps. The weight rows
// [Npad][ldw] as the packer stores them are the MFMA's A operand: lane (row =
// lane & 15, kq = lane >> 4) holds bytes 128 s + 32 kq .. + 31 of its row in K
// step s (two 16-B loads, 2 KB per wave and step), which the MFMA takes as
// K = 32 kq .. 32 kq + 31. The e4m3 batch [B][ldx] is the B operand from the
// same byte positions (images in the 16 columns, zeros beyond B), so both
// operands agree on which K a byte stands for. 8 steps are unrolled: 16 KB of
// weight loads in flight per wave, as in the bf16 kernel (16 steps of 1 KB).
// The waves meet in LDS and one pass sums them in wave order, scales, adds
// the bias, applies ReLU and writes: a fixed summation order, no workspace.
//
// fc_gemm8_kernel (M = B <= 256): fc_gemm.hip's design. A workgroup owns all
// M rows x 128 columns x one K slice; a stage is one K block of 128 (the same
// 128-B LDS rows, 32 KB of activations + 16 KB of weights) brought to a 3-slot
// LDS ring by LDS-DMA, two stages in flight, 16-B chunks XOR-swizzled by row
// through the source addresses. 8 waves = 2 row halves x 4 column quarters:
// 8 x 2 fragments, ONE 16x16x128 MFMA each per stage (the bf16 kernel: two
// 16x16x32 per 64-K stage), so the same stage bytes carry twice the K. A
// lane's operand is chunks fq and fq + 4 of its row: the 16 lanes of a
// ds_read_b128 group (one fq, rows fr = 0..15) then read physical chunks
// (fq ^ (fr & 7)) and that ^ 4, all eight chunk columns twice over rows that
// are 128 B apart, i.e. conflict-free exactly as fc_gemm's chunk 4 kk + fq
// is (sim_topk.hip's FP8 form reads the same pair). Both operands read the
// same chunks, so which K a byte stands for cancels in the sum. Rows >= M read
// the zero page and are never stored. fp32 partials per K slice go to the
// split-K workspace; fc_gemm8_reduce_kernel sums the slices in slice order,
// applies alpha, bias and ReLU and writes bf16 / fp32 / e4m3.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace dmlc {

namespace {

// ---------------------------------------------------------------- output
enum OutKind { kOutBf16 = 0, kOutF32 = 1, kOutE4m3 = 2 };

// t = relu?(sum alpha + bias) as the output type's bits at element o of y
__device__ __forceinline__ void store_out(void* y, long o, float t, int kind, float out_inv_scale) {
  if (kind == kOutF32) {
    ((float*)y)[o] = t;
  } else if (kind == kOutBf16) {
    ((bf16*)y)[o] = f2bf(t);
  } else {
    const float f[4] = {t * out_inv_scale, 0.f, 0.f, 0.f};
    ((uint8_t*)y)[o] = (uint8_t)(e4m3x4_from_f32_clamped(f) & 0xffu);
  }
}

// ---------------------------------------------------------------- quant_e4m3
__global__ __launch_bounds__(256) void quant_e4m3_kernel(const bf16* __restrict__ x, uint8_t* __restrict__ y,
                                                         long groups, float inv_scale) {
  const long g = blockIdx.x * 256L + threadIdx.x;
  if (g >= groups) return;
  float v[8];
  unpack8(*(const uint4*)(x + g * 8), v);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] *= inv_scale;
  u32x2 p;
  p.x = e4m3x4_from_f32_clamped(v);
  p.y = e4m3x4_from_f32_clamped(v + 4);
  *(u32x2*)(y + g * 8) = p;
}

// ---------------------------------------------------------------- fc_small8
constexpr int kUnroll8 = 8;  // K steps (128 k each) with their weight loads in flight per wave (16 KB)
constexpr int kWaves = 8;    // waves per workgroup = K split of one 16-row tile

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

__device__ __forceinline__ v8i load32(const uint8_t* p) {
  const uint4 lo = *(const uint4*)p, hi = *(const uint4*)(p + 16);
  return v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

__global__ __launch_bounds__(64 * kWaves) void fc_small8_kernel(FcSmall8Args a) {
  __shared__ __attribute__((aligned(16))) float part[kWaves][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const int row = lane & 15, kq = lane >> 4;  // A: weight row n0 + row, bytes 32 kq ..; B: image col = row
  const int ksteps = a.K / 128, per = (ksteps + kWaves - 1) / kWaves;
  const int ks0 = min(wave * per, ksteps), ks1 = min(ks0 + per, ksteps);
  const uint8_t* wrow = a.w + (long)(n0 + row) * a.ldw + kq * 32;
  const bool live = row < a.B;
  const uint8_t* xrow = a.x + (long)(live ? row : 0) * a.ldx + kq * 32;
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int ks = ks0; ks < ks1; ks += kUnroll8) {
    v8i wv[kUnroll8], xv[kUnroll8];
#pragma unroll
    for (int u = 0; u < kUnroll8; ++u) {
      const bool in = ks + u < ks1;
      const long k = (long)(in ? ks + u : ks) * 128;  // (a step past the range repeats a valid address, unused)
      const v8i z = {0, 0, 0, 0, 0, 0, 0, 0};
      wv[u] = in ? load32(wrow + k) : z;
      xv[u] = (in && live) ? load32(xrow + k) : z;
    }
#pragma unroll
    for (int u = 0; u < kUnroll8; ++u)
      acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wv[u], xv[u], acc, 0, 0, 0, 127, 0, 127);
  }
  // lane holds D[rows 4 kq .. 4 kq + 3][col = row]: element (r, c) at 16 c + r
  *(floatx4*)&part[wave][row * 16 + 4 * kq] = acc;
  __syncthreads();
  if (tid >= 256) return;
  const int c = tid >> 4, r = tid & 15, n = n0 + r;
  if (c >= a.B || n >= a.N) return;
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s += part[w][tid];
  float t = __builtin_fmaf(s, a.alpha[n], a.bias[n]);
  if (a.relu) t = fmaxf(t, 0.f);
  store_out(a.y, (long)c * a.ldo + n, t, a.out_kind, a.out_inv_scale);
}

// ---------------------------------------------------------------- fc_gemm8
constexpr int kBM = 256;   // rows (images) per workgroup: all of them
constexpr int kBN = 128;   // output columns per workgroup
constexpr int kKB = 128;   // K block per stage: 128 e4m3 bytes a row
constexpr int kAB = kBM * kKB;  // 32 KB A stage
constexpr int kBB = kBN * kKB;  // 16 KB B stage
constexpr int kStage = kAB + kBB;
static_assert(kAB / 1024 == 32 && kBB / 1024 == 16, "6 DMA instructions per wave per stage");
static_assert(3 * kStage <= 160 * 1024, "LDS per CU");

// 16-B chunk c (0..7) of a 128-B LDS row r (fc_gemm.hip's fc_off)
__device__ __forceinline__ int fc_off(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }

__global__ __launch_bounds__(512, 1) void fc_gemm8_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ w,
                                                          float* __restrict__ ws, int M, int K, int Npad, int kslice,
                                                          int nslices, const uint8_t* __restrict__ zero) {
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  char* lds = (char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int fr = lane & 15, fq = lane >> 4;
  // workgroup -> (column block nb, K slice ks): fc_gemm.hip's XCD dealing (with
  // a multiple of 8 slices, XCD x takes slices x, x + 8, ... of every column
  // block, so its L2 holds only its own slices' activations)
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
  const int nstages = kslice / kKB;

  // Staging as in fc_gemm.hip: LDS position p = 64 i + l of a region holds row
  // p >> 3, physical chunk p & 7 = logical chunk (p & 7) ^ (row & 7); a stage
  // is 32 A + 16 B instructions of 1 KB, 6 per wave. Rows >= M read the zero
  // page (which does not advance with K).
  floatx4 acc[8][2];
#pragma unroll
  for (int mf = 0; mf < 8; ++mf)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) acc[mf][nf] = floatx4{0.f, 0.f, 0.f, 0.f};
  const uint8_t* asrc[4];
  const uint8_t* bsrc[2];
  int aoff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = (4 * wave + j) * 64 + lane, r = p >> 3, lc = (p & 7) ^ (r & 7);
    asrc[j] = r < M ? x + (long)r * K + k0 + 16 * lc : zero;
    aoff[j] = r < M ? 1 : 0;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = (2 * wave + j) * 64 + lane, r = p >> 3, lc = (p & 7) ^ (r & 7);
    bsrc[j] = w + (long)(n0 + r) * K + k0 + 16 * lc;
  }
  auto dma_stage = [&](int st, int slot) __attribute__((always_inline)) {
    char* base = lds + slot * kStage;
    const int ko = st * kKB;
#pragma unroll
    for (int j = 0; j < 4; ++j) dma16(asrc[j] + ko * aoff[j], base + (4 * wave + j) * 1024);
#pragma unroll
    for (int j = 0; j < 2; ++j) dma16(bsrc[j] + ko, base + kAB + (2 * wave + j) * 1024);
  };
  // a lane's 32 bytes of row `row`: chunks fq and fq + 4
  auto frag = [&](const char* region, int row) __attribute__((always_inline)) {
    const uint4 lo = *(const uint4*)(region + fc_off(row, fq));
    const uint4 hi = *(const uint4*)(region + fc_off(row, fq + 4));
    return v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  };
  dma_stage(0, 0);
  if (nstages > 1) dma_stage(1, 1);
  for (int s = 0; s < nstages; ++s) {
    // this wave's DMA of stage s has landed (stage s + 1's may stay in
    // flight), after the barrier everyone's has, and every wave is done with
    // stage s - 1, whose slot stage s + 2 reuses
    if (s + 1 < nstages) vm_wait<6>();
    else vm_wait<0>();
    __builtin_amdgcn_s_barrier();
    if (s + 2 < nstages) dma_stage(s + 2, (s + 2) % 3);
    const char* base = lds + (s % 3) * kStage;
    v8i af[8], bf[2];
#pragma unroll
    for (int mf = 0; mf < 8; ++mf) af[mf] = frag(base, 128 * wm + 16 * mf + fr);
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) bf[nf] = frag(base + kAB, 32 * wn + 16 * nf + fr);
#pragma unroll
    for (int mf = 0; mf < 8; ++mf)
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
        acc[mf][nf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[mf], bf[nf], acc[mf][nf], 0, 0, 0, 127, 0, 127);
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

// ws: [splits][M][Npad] fp32. A thread owns 4 consecutive columns of a row
// (N % 4 == 0); the slices are summed in slice order, 8 loads in flight.
__global__ __launch_bounds__(256) void fc_gemm8_reduce_kernel(const float* __restrict__ ws,
                                                              const float* __restrict__ alpha,
                                                              const float* __restrict__ bias, void* __restrict__ y,
                                                              int M, int N, int Npad, int ldo, int splits, int relu,
                                                              int kind, float out_inv_scale) {
  const int n4 = N / 4;
  const long total = (long)M * n4;
  const size_t sstride = (size_t)M * Npad;
  for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int m = (int)(idx / n4);
    const int n = (int)(idx - (long)m * n4) * 4;
    const float* wp = ws + (size_t)m * Npad + n;
    floatx4 s = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 8 <= splits; k += 8) {
      floatx4 t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = *(const floatx4*)(wp + (size_t)(k + u) * sstride);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; k < splits; ++k) s += *(const floatx4*)(wp + (size_t)k * sstride);
    const floatx4 al = *(const floatx4*)(alpha + n), bi = *(const floatx4*)(bias + n);
    float t[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      t[r] = __builtin_fmaf(s[r], al[r], bi[r]);
      if (relu) t[r] = fmaxf(t[r], 0.f);
    }
    const size_t o = (size_t)m * ldo + n;
    if (kind == kOutF32) {
      *(floatx4*)((float*)y + o) = floatx4{t[0], t[1], t[2], t[3]};
    } else if (kind == kOutBf16) {
      *(uint2*)((bf16*)y + o) = make_uint2(pack2(t[0], t[1]), pack2(t[2], t[3]));
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] *= out_inv_scale;
      *(uint32_t*)((uint8_t*)y + o) = e4m3x4_from_f32_clamped(t);
    }
  }
}

int out_kind(bool out_f32, bool out_fp8) {
  if (out_f32 && out_fp8) throw std::invalid_argument("fc8: the output is fp32 or e4m3, not both");
  return out_f32 ? kOutF32 : out_fp8 ? kOutE4m3 : kOutBf16;
}

}  // namespace

void quant_e4m3(const void* x, void* y, int B, int K, float inv_scale, hipStream_t s) {
  if (B < 0 || K < 8 || K % 8) throw std::invalid_argument("quant_e4m3: needs B >= 0, K % 8 == 0, K >= 8");
  if (B == 0) return;
  if (!x || !y || ((uintptr_t)x & 15) || ((uintptr_t)y & 7))
    throw std::invalid_argument("quant_e4m3: null / misaligned operand (x 16 B, y 8 B)");
  if (!(inv_scale > 0.f) || !(inv_scale < INFINITY)) throw std::invalid_argument("quant_e4m3: bad scale");
  const long groups = (long)B * K / 8;
  hipLaunchKernelGGL(quant_e4m3_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, (const bf16*)x,
                     (uint8_t*)y, groups, inv_scale);
  DMLC_HIP_CHECK(hipGetLastError());
}

bool fc_small8_supported(int B, int K, int ldx, int ldw) {
  return B >= 1 && B <= 16 && K >= 128 && K % 128 == 0 && ldx % 16 == 0 && ldw % 16 == 0 && ldw >= K && ldx >= K;
}

void fc_small8(const void* x, int ldx, const void* w, int ldw, const float* alpha, const float* bias, void* y, int ldo,
               bool out_f32, bool out_fp8, float out_inv_scale, int B, int K, int N, int Npad, bool relu,
               hipStream_t s) {
  if (B <= 0) return;
  if (!fc_small8_supported(B, K, ldx, ldw) || N < 1 || Npad < ((N + 15) / 16) * 16 || ldo < N)
    throw std::invalid_argument("fc_small8: unsupported shape");
  if (!x || !w || !alpha || !bias || !y || (((uintptr_t)x | (uintptr_t)w) & 15))
    throw std::invalid_argument("fc_small8: null / misaligned operand");
  FcSmall8Args a;
  a.x = (const uint8_t*)x;
  a.w = (const uint8_t*)w;
  a.alpha = alpha;
  a.bias = bias;
  a.y = y;
  a.B = B;
  a.K = K;
  a.N = N;
  a.ldx = ldx;
  a.ldw = ldw;
  a.ldo = ldo;
  a.relu = relu;
  a.out_kind = out_kind(out_f32, out_fp8);
  a.out_inv_scale = out_fp8 ? out_inv_scale : 1.f;
  hipLaunchKernelGGL(fc_small8_kernel, dim3((N + 15) / 16), dim3(64 * kWaves), 0, s, a);
  DMLC_HIP_CHECK(hipGetLastError());
}

int fc_gemm8_splits(const ConvArgs& a, int num_cus) {
  if (a.Kpad <= 0 || a.Npad <= 0 || a.Npad % kBN) return 0;
  const int kb = a.Kpad / kKB;
  const int cols = a.Npad / kBN;
  // fc_gemm_splits' rule in 128-K blocks: about one workgroup per CU, each at least 4 K blocks
  int s = std::max(1, std::min(kb / 4, (num_cus + cols - 1) / cols));
  while (s > 1 && kb % s) --s;  // whole K blocks per slice
  return s;
}

bool fc_gemm8_supported(const ConvArgs& a) {
  return a.H == 1 && a.W == 1 && a.KH == 1 && a.KW == 1 && a.Ho == 1 && a.Wo == 1 && !a.stem && a.in_fp8 &&
         !(a.out_f32 && a.out_fp8) && !a.res && a.B >= 1 && a.B <= kBM && a.Cin == a.Kpad && a.Kpad >= kKB &&
         a.Kpad % kKB == 0 && a.Npad >= kBN && a.Npad % kBN == 0 && a.N >= 4 && a.N % 4 == 0 && a.N <= a.Npad &&
         a.ldo >= a.N && a.ldo % 4 == 0;
}

void fc_gemm8(const ConvArgs& a, int splits, hipStream_t s) {
  if (!fc_gemm8_supported(a)) throw std::invalid_argument("fc_gemm8: unsupported layer");
  if (splits < 1 || (a.Kpad / kKB) % splits) throw std::invalid_argument("fc_gemm8: K blocks must split evenly");
  if (!a.x || !a.w || !a.y || !a.zero || !a.ws || !a.alpha || !a.bias ||
      (((uintptr_t)a.x | (uintptr_t)a.w | (uintptr_t)a.zero | (uintptr_t)a.y | (uintptr_t)a.ws | (uintptr_t)a.alpha |
        (uintptr_t)a.bias) & 15))
    throw std::invalid_argument("fc_gemm8: null / misaligned operand (the workspace, alpha and bias are required)");
  const int M = a.B;
  const int kslice = a.Kpad / splits;
  hipLaunchKernelGGL(fc_gemm8_kernel, dim3(a.Npad / kBN * splits), dim3(512), (size_t)3 * kStage, s,
                     (const uint8_t*)a.x, (const uint8_t*)a.w, a.ws, M, a.Kpad, a.Npad, kslice, splits,
                     (const uint8_t*)a.zero);
  DMLC_HIP_CHECK(hipGetLastError());
  const int blocks = (int)std::min<long>(((long)M * (a.N / 4) + 255) / 256, 4096);
  hipLaunchKernelGGL(fc_gemm8_reduce_kernel, dim3(blocks), dim3(256), 0, s, (const float*)a.ws, a.alpha, a.bias, a.y, M,
                     a.N, a.Npad, a.ldo, splits, (int)a.relu, out_kind(a.out_f32, a.out_fp8),
                     a.out_fp8 ? a.out_inv_scale : 1.f);
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
