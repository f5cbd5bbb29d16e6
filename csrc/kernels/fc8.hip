// Fully connected layers on e4m3 (OCP, one byte per weight): AlexNet's
// classifier.1 / classifier.4 of the `alexnet_fp8` arch. The FP8 = true
// instantiations of fc_kernels.h (the designs are described there), the
// activation quantiser, the e4m3 forms' own finish and their entry points.
//
// y[b][n] = act((sum_k cx[b][k] cw[n][k]) alpha[n] + bias[n]), cx / cw the
// e4m3 codes, alpha[n] = s_x s_w[n] (the activation's per-tensor scale times
// the weight row's), written as bf16, fp32 or e4m3(y out_inv_scale)
// (saturating, common.h's clamped converter).
//
// quant_e4m3_kernel: bf16 rows -> e4m3(v inv_scale). A thread owns 8 values:
// one 16-B load, one 8-B store.
//
// fc_gemm8_reduce_kernel sums fc_gemm_kernel<true>'s fp32 partials in slice
// order, applies alpha, bias and ReLU and writes bf16 / fp32 / e4m3.
//
// Compiled without packed fp32 VALU ops (tools/build.py).
#include <cmath>

#include "fc_kernels.h"

namespace dmlc {

namespace {

constexpr int kKB = kFcKB<true>;

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

// ---------------------------------------------------------------- fc_gemm8's reduction
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
  hipLaunchKernelGGL(fc_small_kernel<true>, dim3((N + 15) / 16), dim3(64 * kWaves), 0, s, a);
  DMLC_HIP_CHECK(hipGetLastError());
}

int fc_gemm8_splits(const ConvArgs& a, int num_cus) { return fc_gemm_splits_rule<true>(a, num_cus); }

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
  fc_gemm_launch<true>(a, splits, s);
  const int M = a.B;
  const int blocks = (int)std::min<long>(((long)M * (a.N / 4) + 255) / 256, 4096);
  hipLaunchKernelGGL(fc_gemm8_reduce_kernel, dim3(blocks), dim3(256), 0, s, (const float*)a.ws, a.alpha, a.bias, a.y, M,
                     a.N, a.Npad, a.ldo, splits, (int)a.relu, out_kind(a.out_f32, a.out_fp8),
                     a.out_fp8 ? a.out_inv_scale : 1.f);
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
