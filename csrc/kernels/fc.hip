// Fully connected layers on bf16: the FP8 = false instantiations of
// fc_kernels.h (the designs are described there) and their entry points.
// fc_small writes bf16 / fp32 itself; fc_gemm's fp32 partials per K slice are
// reduced (+ bias, ReLU, bf16 / fp32 out) by conv_igemm.hip's splitk_reduce.
#include "fc_kernels.h"

namespace dmlc {

namespace {
constexpr int kKB = kFcKB<false>;
}

bool fc_small_supported(int B, int K, int ldx, int ldw) {
  return B >= 1 && B <= 16 && K % 32 == 0 && ldx % 8 == 0 && ldw % 8 == 0 && ldw >= K && ldx >= K;
}

void fc_small(const void* x, int ldx, const void* w, int ldw, const float* bias, void* y, int ldo, bool out_f32,
              int B, int K, int N, int Npad, bool relu, hipStream_t s) {
  if (B <= 0) return;
  if (!fc_small_supported(B, K, ldx, ldw) || Npad < ((N + 15) / 16) * 16)
    throw std::invalid_argument("fc_small: unsupported shape");
  if (!x || !w || !bias || !y || (((uintptr_t)x | (uintptr_t)w) & 15))
    throw std::invalid_argument("fc_small: null / misaligned operand");
  FcSmallArgs a;
  a.x = (const bf16*)x;
  a.w = (const bf16*)w;
  a.bias = bias;
  a.y = y;
  a.B = B;
  a.K = K;
  a.N = N;
  a.ldx = ldx;
  a.ldw = ldw;
  a.ldo = ldo;
  a.relu = relu;
  a.out_f32 = out_f32;
  hipLaunchKernelGGL(fc_small_kernel<false>, dim3((N + 15) / 16), dim3(64 * kWaves), 0, s, a);
  DMLC_HIP_CHECK(hipGetLastError());
}

int fc_gemm_splits(const ConvArgs& a, int num_cus) { return fc_gemm_splits_rule<false>(a, num_cus); }

bool fc_gemm_supported(const ConvArgs& a) {
  return a.H == 1 && a.W == 1 && a.KH == 1 && a.KW == 1 && a.Ho == 1 && a.Wo == 1 && !a.stem && !a.in_fp8 &&
         !a.out_fp8 && !a.res && a.B >= 1 && a.B <= kBM && a.Cin == a.Kpad && a.Kpad % kKB == 0 &&
         a.Npad % kBN == 0 && a.N <= a.Npad;
}

void fc_gemm(const ConvArgs& a, int splits, hipStream_t s) {
  if (!fc_gemm_supported(a)) throw std::invalid_argument("fc_gemm: unsupported layer");
  if (splits < 1 || (a.Kpad / kKB) % splits) throw std::invalid_argument("fc_gemm: K blocks must split evenly");
  if (!a.x || !a.w || !a.y || !a.zero || !a.ws || (((uintptr_t)a.x | (uintptr_t)a.w | (uintptr_t)a.zero) & 15))
    throw std::invalid_argument("fc_gemm: null / misaligned operand (the workspace is required)");
  fc_gemm_launch<false>(a, splits, s);
  ConvArgs b = a;
  b.split_k = splits;
  splitk_reduce(b, a.B, splits, s);
}

}  // namespace dmlc
