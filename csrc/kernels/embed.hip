// Penultimate-layer embeddings: the vector the classifier's last fc reads, as
// fp32 rows, optionally scaled to unit L2 norm.
//
// Reference counterpart: none. The reference answers with a class name only
// (src/services.rs:493-497); this is what torch users take from a hook on
// `avgpool` or a model built with num_classes = 0.
//
// x is [B, HW, C] bf16, or e4m3 with a per-tensor scale (HW > 1); out is
// fp32 [B, C], dense. Two stages:
//
// 1. v[b, c]. HW == 1: the bf16 element widened (exact). HW > 1: the global
//    average exactly as avgpool_global computes it (pool.hip; its two kernels
//    agree bit for bit): fp32 part sums, part p adding pixels p, p + 8, ... in
//    order onto +0; the 8 parts combined as ((0+1)+(2+3))+((4+5)+(6+7)); one
//    multiply by (in_fp8 ? scale : 1) / HW; rounded to bf16 (nearest even) and
//    widened. So v is always the bf16 number the fc multiplies, whichever
//    batch path of the engine produced or skipped it.
// 2. out = v, or with l2norm v / max(sqrt(sum_c v^2), 1e-12) (torch's
//    F.normalize with its default eps): fp32 squares summed per lane, across
//    the wave, then across the workgroup's waves through LDS; an IEEE square
//    root and division. An all-zero row gives zeros. There is no overflow
//    guard: a row with |v| > 1.8e19 has an infinite sum of squares and comes
//    out as zeros (or NaN where v is infinite).
//
// Memory-bound. One workgroup per image; a lane owns 8-channel groups tid,
// tid + nt, ... (at most kMaxGroups of them, C <= 8192), so a wave reads 512
// contiguous channels of a pixel per load (16 B a lane, 8 B for e4m3) and
// writes 2 KB of contiguous fp32 (two 16-B stores a lane). The HW > 1 form
// issues its loads in blocks of 24 pixels, as avgpool_rows_kernel does. A
// lane keeps its v in registers between the two stages: x is read once.
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace dmlc {

namespace {

constexpr int kMaxC = 8192;
constexpr int kThreads = 256;
constexpr int kMaxGroups = kMaxC / 8 / kThreads;  // 8-channel groups per lane at the widest row

// avgpool_rows_kernel's body for one 8-channel group (base = its first pixel)
template <bool FP8>
__device__ __forceinline__ void pool_group(const void* __restrict__ xv, long base, int HW, int C, float inv,
                                           float* __restrict__ o) {
  float s[8][8];
#pragma unroll
  for (int p = 0; p < 8; ++p)
#pragma unroll
    for (int j = 0; j < 8; ++j) s[p][j] = 0.f;
  constexpr int BLK = 24;
  for (int i0 = 0; i0 < HW; i0 += BLK) {
    uint4 v[BLK];
#pragma unroll
    for (int u = 0; u < BLK; ++u) {
      const int i = i0 + u;
      if (i < HW) {
        if constexpr (FP8) {
          const uint2 q = *(const uint2*)((const uint8_t*)xv + base + (long)i * C);
          v[u] = make_uint4(q.x, q.y, 0u, 0u);
        } else {
          v[u] = *(const uint4*)((const bf16*)xv + base + (long)i * C);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < BLK; ++u) {
      const int i = i0 + u;
      if (i < HW) {
        float f[8];
        if constexpr (FP8) {
          e4m3x4_to_f32((uint32_t)v[u].x, f);
          e4m3x4_to_f32((uint32_t)v[u].y, f + 4);
        } else {
          unpack8(v[u], f);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) s[u & 7][j] += f[j];  // (BLK % 8 == 0: part = i % 8 = u % 8)
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = (((s[0][j] + s[1][j]) + (s[2][j] + s[3][j])) + ((s[4][j] + s[5][j]) + (s[6][j] + s[7][j]))) * inv;
    o[j] = bf2f(f2bf(a));
  }
}

// POOL: HW > 1. blockDim.x = nt (a multiple of 64, <= kThreads), C <= 8 * nt * kMaxGroups.
template <bool FP8, bool POOL>
__global__ __launch_bounds__(kThreads) void embed_rows_kernel(const void* __restrict__ xv, float* __restrict__ out,
                                                              int HW, int C, float scale, int l2norm) {
  __shared__ float wsum[kThreads / 64];
  const int b = blockIdx.x;
  const int nt = blockDim.x;
  const int c8 = C / 8;
  const float inv = (FP8 ? scale : 1.f) / HW;
  float v[kMaxGroups][8];
  float ss = 0.f;
#pragma unroll
  for (int g = 0; g < kMaxGroups; ++g) {
    const int cg = threadIdx.x + g * nt;
    if (cg < c8) {
      if constexpr (POOL) {
        pool_group<FP8>(xv, (long)b * HW * C + cg * 8, HW, C, inv, v[g]);
      } else {
        unpack8(*(const uint4*)((const bf16*)xv + (long)b * C + cg * 8), v[g]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += v[g][j] * v[g][j];
    }
  }
  float r = 1.f;
  if (l2norm) {  // (uniform over the workgroup)
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = ss;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < nt / 64; ++w) t += wsum[w];
    r = fmaxf(sqrtf(t), 1e-12f);
  }
#pragma unroll
  for (int g = 0; g < kMaxGroups; ++g) {
    const int cg = threadIdx.x + g * nt;
    if (cg < c8) {
      float4 lo, hi;
      if (l2norm) {
        lo = make_float4(v[g][0] / r, v[g][1] / r, v[g][2] / r, v[g][3] / r);
        hi = make_float4(v[g][4] / r, v[g][5] / r, v[g][6] / r, v[g][7] / r);
      } else {
        lo = make_float4(v[g][0], v[g][1], v[g][2], v[g][3]);
        hi = make_float4(v[g][4], v[g][5], v[g][6], v[g][7]);
      }
      float4* o = (float4*)(out + (long)b * C + cg * 8);
      o[0] = lo;
      o[1] = hi;
    }
  }
}

}  // namespace

bool embed_rows_supported(int HW, int C) { return HW >= 1 && C >= 8 && C % 8 == 0 && C <= kMaxC; }

void embed_rows(const void* x, float* out, int B, int HW, int C, bool in_fp8, float scale, bool l2norm,
                hipStream_t s) {
  if (!embed_rows_supported(HW, C)) throw std::invalid_argument("embed_rows: needs HW >= 1, C % 8 == 0, C <= 8192");
  if (in_fp8 && HW == 1) throw std::invalid_argument("embed_rows: an e4m3 input needs HW > 1");
  if (B < 0) throw std::invalid_argument("embed_rows: B < 0");
  if (B == 0) return;
  if (!x || !out) throw std::invalid_argument("embed_rows: null x / out");
  if ((uintptr_t)x % (in_fp8 ? 8 : 16) || (uintptr_t)out % 16)
    throw std::invalid_argument("embed_rows: x needs 16-B alignment (8-B for e4m3) and out 16-B");
  // whole waves, enough of them for the row's channel groups
  const int c8 = C / 8, nt = std::min((c8 + 63) / 64 * 64, kThreads);
  static_assert(kMaxGroups * kThreads * 8 == kMaxC, "a lane's groups cover the widest row");
  const dim3 grid(B), block(nt);
  const int n = l2norm ? 1 : 0;
  if (HW == 1)
    hipLaunchKernelGGL((embed_rows_kernel<false, false>), grid, block, 0, s, x, out, HW, C, 1.f, n);
  else if (in_fp8)
    hipLaunchKernelGGL((embed_rows_kernel<true, true>), grid, block, 0, s, x, out, HW, C, scale, n);
  else
    hipLaunchKernelGGL((embed_rows_kernel<false, true>), grid, block, 0, s, x, out, HW, C, 1.f, n);
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
