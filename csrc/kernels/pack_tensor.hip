// Float tensor -> the conv stem's packed bf16 image: the layout preprocess_u8
// writes (preprocess.hip), from values the caller already normalised.
//
// x is [B, 3, S, S] (NCHW) or [B, S, S, 3] (channels_last) in fp32, fp16 or
// bf16. y is [B, S+2p, Wr, 3] bf16 with the image at (p, p), or the paired form
// [B, S+2p, Wr/2, 8] with 16-B chunks [r g b r g b 0 0]. No resize, no
// normalisation, no clamping: every value is rounded to bf16 (nearest even;
// fp16 through fp32, bf16 copied bit for bit) and every other byte of y is
// written as zero on every launch, since the stem reads the border without
// bounds checks and the arena is reused.
//
// One thread writes 8 consecutive pixels of an output row as three (paired:
// four) 16-B stores; Wr % 8 == 0 keeps every store aligned. Its reads are
// element loads: with pad = 3 the image starts 3 elements off the store grid
// and rows of S elements follow each other with no padding, so nothing wider
// than the element is aligned. With NCHW a thread reads 8 consecutive
// elements of each of the three planes and the next thread the next 8, so a
// wave's 24 loads cover three contiguous runs of 512 elements, each cache
// line used whole; with channels_last the 24 elements of a thread are one
// contiguous run.
#include "common.h"
#include "kernels.h"

#include <hip/hip_fp16.h>

#include <algorithm>

namespace dmlc {

namespace {

struct PackParams {
  int B, S, pad, P, Wr;  // P = S + 2*pad rows, Wr pixels per row
};

__device__ __forceinline__ uint32_t bf16_bits(float v) { return __builtin_bit_cast(uint16_t, f2bf(v)); }
__device__ __forceinline__ uint32_t bf16_bits(__half v) { return bf16_bits(__half2float(v)); }
__device__ __forceinline__ uint32_t bf16_bits(bf16 v) { return __builtin_bit_cast(uint16_t, v); }

template <typename T, bool CL, bool PAIRED>
__global__ __launch_bounds__(256) void pack_tensor_kernel(const T* __restrict__ x, uint4* __restrict__ y,
                                                          PackParams p) {
  const int groups = p.Wr / 8;
  const long total = (long)p.B * p.P * groups;
  const long plane = (long)p.S * p.S;
  for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int g = (int)(idx % groups);
    const long t = idx / groups;
    const int hy = (int)(t % p.P);
    const int b = (int)(t / p.P);
    const int iy = hy - p.pad;
    const int x0 = g * 8 - p.pad;
    uint32_t h[24];  // bf16 bits, pixel-major: h[3 i + c]
#pragma unroll
    for (int i = 0; i < 24; ++i) h[i] = 0;
    if ((unsigned)iy < (unsigned)p.S && x0 + 8 > 0 && x0 < p.S) {
      const T* img = x + (long)b * 3 * plane;
      const long row = (long)iy * p.S;
      if (x0 >= 0 && x0 + 8 <= p.S) {  // the whole group inside the image: 24 loads in flight, no masks
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int c = 0; c < 3; ++c)
            h[3 * i + c] = bf16_bits(CL ? img[(row + x0 + i) * 3 + c] : img[c * plane + row + x0 + i]);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int ix = x0 + i;
          if ((unsigned)ix < (unsigned)p.S) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
              h[3 * i + c] = bf16_bits(CL ? img[(row + ix) * 3 + c] : img[c * plane + row + ix]);
          }
        }
      }
    }
    if (PAIRED) {
      uint4* dst = y + idx * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t* v = h + 6 * q;
        dst[q] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), 0u);
      }
    } else {
      uint4* dst = y + idx * 3;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const uint32_t* v = h + 8 * q;
        dst[q] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
      }
    }
  }
}

template <typename T>
void launch(const void* x, bool channels_last, bool paired, void* y, const PackParams& p, int blocks,
            hipStream_t s) {
  const T* xt = (const T*)x;
  uint4* yt = (uint4*)y;
  if (channels_last) {
    if (paired)
      hipLaunchKernelGGL((pack_tensor_kernel<T, true, true>), dim3(blocks), dim3(256), 0, s, xt, yt, p);
    else
      hipLaunchKernelGGL((pack_tensor_kernel<T, true, false>), dim3(blocks), dim3(256), 0, s, xt, yt, p);
  } else {
    if (paired)
      hipLaunchKernelGGL((pack_tensor_kernel<T, false, true>), dim3(blocks), dim3(256), 0, s, xt, yt, p);
    else
      hipLaunchKernelGGL((pack_tensor_kernel<T, false, false>), dim3(blocks), dim3(256), 0, s, xt, yt, p);
  }
}

}  // namespace

size_t tensor_dtype_bytes(TensorDType dt) { return dt == TensorDType::F32 ? 4 : 2; }

void pack_tensor(const void* x, TensorDType dt, bool channels_last, void* y, int B, int S, int pad, int Wr,
                 bool paired, hipStream_t s) {
  if (dt != TensorDType::F32 && dt != TensorDType::F16 && dt != TensorDType::BF16)
    throw std::invalid_argument("pack_tensor: unknown dtype");
  if (B < 0 || S <= 0 || pad < 0 || Wr < S + 2 * pad || Wr % 8 != 0) throw std::invalid_argument("pack_tensor: bad dims");
  if (!x || !y || ((uintptr_t)y & 15) || ((uintptr_t)x & (tensor_dtype_bytes(dt) - 1)))
    throw std::invalid_argument("pack_tensor: null / misaligned operand");
  if (B == 0) return;
  PackParams p;
  p.B = B;
  p.S = S;
  p.pad = pad;
  p.P = S + 2 * pad;
  p.Wr = Wr;
  const long total = (long)B * p.P * (Wr / 8);
  const int blocks = (int)std::min<long>((total + 255) / 256, 16384);
  switch (dt) {
    case TensorDType::F32:
      launch<float>(x, channels_last, paired, y, p, blocks, s);
      break;
    case TensorDType::F16:
      launch<__half>(x, channels_last, paired, y, p, blocks, s);
      break;
    case TensorDType::BF16:
      launch<bf16>(x, channels_last, paired, y, p, blocks, s);
      break;
  }
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
