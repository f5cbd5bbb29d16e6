// Fused softmax + top-k over the classifier logits.
//
// Reference: `forward_t(..).softmax(-1)` then `imagenet::top(output, k)`
// (src/model_utils.rs:19,42; the services call it with k = 1). One wave per
// row, four rows per workgroup, as softmax_top1: no LDS, nothing shared
// between waves.
//
// Order: the k largest logits of columns 0..N-1 in descending order, equal
// logits by ascending class index (softmax_top1's tie rule at every rank).
// Probabilities: exp(x_j - max) / sum_i exp(x_i - max), the sum taken exactly
// as softmax_top1 takes it (per-lane partial sums over i = lane, lane + 64,
// ..., then wave_sum), so rank 0 is bit-equal to softmax_top1 for any k.
// Logits are assumed finite: -inf marks an empty or retired slot, and a NaN
// never wins a comparison.
//
// Rows of up to kRegN = 64 * kRegVals = 1024 columns (the 1000 ImageNet
// classes) are read once: every lane keeps its strided share in kRegVals
// registers, and each of the k rounds is a per-lane arg-max over those
// registers, a (value, index) butterfly across the wave, and the winner's
// slot set to -inf in the lane that owns it. Longer rows would not fit the
// register budget with static indexing; they run k rounds that each reread
// the (L2-resident) row and take the best element that sorts after the
// previous round's winner.
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace dmlc {

namespace {

constexpr int kRegVals = 16;
constexpr int kRegN = 64 * kRegVals;

// (v, i) across the wave: the largest value, the lowest index among equals
__device__ __forceinline__ void wave_argmax(float& best, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
}

template <bool REG>
__global__ __launch_bounds__(256) void softmax_topk_kernel(const float* __restrict__ logits, int B, int N, int ld,
                                                           int k, int32_t* __restrict__ idx,
                                                           float* __restrict__ prob) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const float* p = logits + (long)row * ld;
  float v[kRegVals];
  if constexpr (REG) {
#pragma unroll
    for (int j = 0; j < kRegVals; ++j) {
      const int i = lane + 64 * j;
      v[j] = i < N ? p[i] : -INFINITY;
    }
  }
  float top = 0.f, s = 0.f;           // the row maximum and the exp-sum (set in round 0)
  float pv = INFINITY;                // rereading rows: the previous winner
  int pi = -1;
  int my_i = 0;                       // lane r keeps rank r
  float my_v = 0.f;
  for (int r = 0; r < k; ++r) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if constexpr (REG) {
#pragma unroll
      for (int j = 0; j < kRegVals; ++j)
        if (v[j] > best) {  // the index grows with j, so the first maximum wins within a lane
          best = v[j];
          bi = lane + 64 * j;
        }
    } else {
      for (int i = lane; i < N; i += 64) {
        const float x = p[i];
        const bool after = x < pv || (x == pv && i > pi);  // sorts after the previous winner
        if (after && x > best) {
          best = x;
          bi = i;
        }
      }
    }
    wave_argmax(best, bi);
    if (r == 0) {
      top = best;
      if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < kRegVals; ++j)
          if (lane + 64 * j < N) s += __expf(v[j] - top);
      } else {
        for (int i = lane; i < N; i += 64) s += __expf(p[i] - top);
      }
      s = wave_sum(s);
    }
    if constexpr (REG) {
#pragma unroll
      for (int j = 0; j < kRegVals; ++j)
        if (bi == lane + 64 * j) v[j] = -INFINITY;
    } else {
      pv = best;
      pi = bi;
    }
    if (lane == r) {
      my_i = bi;
      my_v = best;
    }
  }
  if (lane < k) {
    idx[(long)row * k + lane] = my_i;
    prob[(long)row * k + lane] = lane == 0 ? 1.f / s : __expf(my_v - top) / s;
  }
}

}  // namespace

void softmax_topk(const float* logits, int B, int N, int ld, int k, int32_t* idx, float* prob, hipStream_t s) {
  if (B <= 0) return;
  if (N <= 0 || ld < N) throw std::invalid_argument("softmax_topk: bad N/ld");
  if (k < 1 || k > N || k > kMaxTopK) throw std::invalid_argument("softmax_topk: k must be in 1..min(N, kMaxTopK)");
  static_assert(kMaxTopK <= 64, "one lane per rank");
  const dim3 grid((B + 3) / 4), block(256);
  if (N <= kRegN)
    hipLaunchKernelGGL(softmax_topk_kernel<true>, grid, block, 0, s, logits, B, N, ld, k, idx, prob);
  else
    hipLaunchKernelGGL(softmax_topk_kernel<false>, grid, block, 0, s, logits, B, N, ld, k, idx, prob);
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
