// Ragged batch resize: differently sized u8 HWC images -> one u8 [B, S, S, 3]
// batch, so a query of mixed-size JPEGs becomes ONE (graph-replayed) forward
// instead of one forward per distinct size.
//
// Reference equivalent: tch `imagenet::load_image_and_resize(path, 224, 224)`
// per query (src/services.rs:492), which resizes the decoded image to u8
// before normalising. Same rule as preprocess.hip (short side -> S, long side
// floor(S*long/short), centre crop, bilinear with half-pixel centres), with the
// result rounded to u8; normalisation then happens inside the fused stem
// (stem_pool.hip) of the forward.
//
// Each image comes from a descriptor {pointer, H, W} in device memory (the
// decoded images live in the executor's HBM cache at their own sizes). One
// thread writes 4 consecutive pixels = 12 B as three dword stores; grid =
// (pixel blocks, B).
//
// resize_ragged_aa_kernel (antialias = true) is the same geometry with a
// triangle filter whose support is stretched by max(scale, 1) per axis (PIL's
// and torch's antialias=True bilinear), so shrinking averages every source
// pixel instead of sampling four. The tap count grows with the scale and is a
// run-time quantity, so the filter is separable: a block owns kAaRows output
// rows x kAaCols output columns (one column per lane), walks the source rows
// those output rows touch once, filters each horizontally (each lane over its
// own taps, straight from global memory: neighbouring lanes' taps overlap, so
// the lines come from L1/L2) and adds the filtered row into the output rows it
// contributes to. fp32 throughout, one rounding to u8 at the end. The u8 tile
// goes through LDS so that the stores are the same 12 B per thread.
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace dmlc {

namespace {

__global__ __launch_bounds__(256) void resize_ragged_kernel(const ImageDesc* __restrict__ descs,
                                                            uint8_t* __restrict__ out, int S) {
  const int b = blockIdx.y;
  const ImageDesc d = descs[b];
  const int q = blockIdx.x * 256 + threadIdx.x;  // quad of pixels
  const int quads = S * S / 4;
  if (q >= quads) return;
  const int p0 = q * 4;
  const int y = p0 / S, x0 = p0 % S;
  uint8_t v[12];
  if (d.h == S && d.w == S) {
    const uint8_t* src = d.ptr + ((long)y * S + x0) * 3;
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = src[i];
  } else {
    int RH, RW;
    if (d.h <= d.w) {
      RH = S;
      RW = (int)((long)S * d.w / d.h);
    } else {
      RW = S;
      RH = (int)((long)S * d.h / d.w);
    }
    const float sys = (float)d.h / RH, sxs = (float)d.w / RW;
    const int oy = (RH - S) / 2, ox = (RW - S) / 2;
    float sy = (y + oy + 0.5f) * sys - 0.5f;
    sy = fminf(fmaxf(sy, 0.f), (float)(d.h - 1));
    const int y0 = (int)sy, y1 = min(y0 + 1, d.h - 1);
    const float fy = sy - y0;
    const uint8_t* r0 = d.ptr + (long)y0 * d.w * 3;
    const uint8_t* r1 = d.ptr + (long)y1 * d.w * 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float sx = (x0 + i + ox + 0.5f) * sxs - 0.5f;
      sx = fminf(fmaxf(sx, 0.f), (float)(d.w - 1));
      const int xa = (int)sx, xb = min(xa + 1, d.w - 1);
      const float fx = sx - xa;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float a = r0[xa * 3 + k], bb = r0[xb * 3 + k], c = r1[xa * 3 + k], e = r1[xb * 3 + k];
        const float top = a + (bb - a) * fx, bot = c + (e - c) * fx;
        const float val = top + (bot - top) * fy;
        v[i * 3 + k] = (uint8_t)fminf(fmaxf(rintf(val), 0.f), 255.f);
      }
    }
  }
  uint32_t* dst = (uint32_t*)(out + ((long)b * S * S + p0) * 3);
#pragma unroll
  for (int i = 0; i < 3; ++i)
    dst[i] = (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) | ((uint32_t)v[4 * i + 2] << 16) |
             ((uint32_t)v[4 * i + 3] << 24);
}

constexpr int kAaRows = 8;   // output rows per block
constexpr int kAaCols = 64;  // output columns per block: one per lane of the wave

// One axis of the antialiased filter for output index i (before the crop) of
// n_in -> n_out: centre, 1 / support and the taps [lo, hi), all inside [0, n_in).
struct AaAxis {
  float c, inv_sup;
  int lo, hi;
};

__device__ __forceinline__ AaAxis aa_axis(int i, int n_in, int n_out) {
  const float scale = (float)n_in / (float)n_out, sup = fmaxf(scale, 1.f);
  AaAxis a;
  a.c = scale * (i + 0.5f);
  a.inv_sup = 1.f / sup;
  a.lo = max(0, (int)(a.c - sup + 0.5f));
  a.hi = min(n_in, (int)(a.c + sup + 0.5f));
  return a;
}

__device__ __forceinline__ float aa_weight(const AaAxis& a, int j) {
  return fmaxf(0.f, 1.f - fabsf((j - a.c + 0.5f) * a.inv_sup));
}

__device__ __forceinline__ float aa_inv_norm(const AaAxis& a) {
  float t = 0.f;
  for (int j = a.lo; j < a.hi; ++j) t += aa_weight(a, j);
  return t > 0.f ? 1.f / t : 0.f;
}

__global__ __launch_bounds__(kAaCols) void resize_ragged_aa_kernel(const ImageDesc* __restrict__ descs,
                                                                  uint8_t* __restrict__ out, int S) {
  __shared__ uint32_t tile[kAaRows][kAaCols * 3 / 4];  // u8 [kAaRows][kAaCols][3]
  uint8_t* t8 = (uint8_t*)&tile[0][0];
  const int b = blockIdx.z, lane = threadIdx.x;
  const ImageDesc d = descs[b];
  const int x0 = blockIdx.x * kAaCols, y0 = blockIdx.y * kAaRows;
  const int rows = min(kAaRows, S - y0), cols = min(kAaCols, S - x0);  // (cols % 4 == 0)
  const int x = x0 + lane;
  const int qpr = cols / 4;  // 12-byte groups per tile row
  if (d.h == S && d.w == S) {
    // copy, as resize_ragged_kernel does it: 12 B per thread straight through
    // (the same for the whole block, so nobody is left waiting at the barrier)
    for (int i = lane; i < rows * qpr; i += kAaCols) {
      const int k = i / qpr, q = i - k * qpr;
      const long p = (((long)(y0 + k)) * S + x0 + q * 4) * 3;
      const uint8_t* src = d.ptr + p;
      uint8_t v[12];
#pragma unroll
      for (int c = 0; c < 12; ++c) v[c] = src[c];
      uint32_t* dst = (uint32_t*)(out + (long)b * S * S * 3 + p);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        dst[c] = (uint32_t)v[4 * c] | ((uint32_t)v[4 * c + 1] << 8) | ((uint32_t)v[4 * c + 2] << 16) |
                 ((uint32_t)v[4 * c + 3] << 24);
    }
    return;
  }
  {  // (the accumulators live only up to the LDS tile)
    float acc[kAaRows][3];
#pragma unroll
    for (int k = 0; k < kAaRows; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.f;
    if (lane < cols && d.h > 0 && d.w > 0) {
      int RH, RW;
      if (d.h <= d.w) {
        RH = S;
        RW = (int)((long)S * d.w / d.h);
      } else {
        RW = S;
        RH = (int)((long)S * d.h / d.w);
      }
      const int oy = (RH - S) / 2, ox = (RW - S) / 2;
      const AaAxis ax = aa_axis(x + ox, d.w, RW);
      const float inx = aa_inv_norm(ax);
      // (rows past the tile's last one repeat it: same source rows, never stored)
      AaAxis ay[kAaRows];
      float iny[kAaRows];
#pragma unroll
      for (int k = 0; k < kAaRows; ++k) {
        ay[k] = aa_axis(y0 + min(k, rows - 1) + oy, d.h, RH);
        iny[k] = aa_inv_norm(ay[k]);
      }
      const int r_end = aa_axis(y0 + rows - 1 + oy, d.h, RH).hi;
      for (int r = ay[0].lo; r < r_end; ++r) {  // every read: 0 <= r < d.h, 0 <= j < d.w
        const uint8_t* row = d.ptr + (long)r * d.w * 3;
        float h0 = 0.f, h1 = 0.f, h2 = 0.f;
        for (int j = ax.lo; j < ax.hi; ++j) {
          const float wx = aa_weight(ax, j);
          const uint8_t* p = row + j * 3;
          h0 += wx * p[0];
          h1 += wx * p[1];
          h2 += wx * p[2];
        }
        h0 *= inx;
        h1 *= inx;
        h2 *= inx;
#pragma unroll
        for (int k = 0; k < kAaRows; ++k) {
          const float wy = (r >= ay[k].lo && r < ay[k].hi) ? aa_weight(ay[k], r) * iny[k] : 0.f;
          acc[k][0] += wy * h0;
          acc[k][1] += wy * h1;
          acc[k][2] += wy * h2;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kAaRows; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        t8[(k * kAaCols + lane) * 3 + c] = (uint8_t)fminf(fmaxf(rintf(acc[k][c]), 0.f), 255.f);
  }
  __syncthreads();
  for (int i = lane; i < rows * qpr; i += kAaCols) {
    const int k = i / qpr, q = i - k * qpr;
    const uint32_t* src = &tile[k][q * 3];
    uint32_t* dst = (uint32_t*)(out + (((long)b * S + y0 + k) * S + x0 + q * 4) * 3);
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
  }
}

}  // namespace

void resize_u8_ragged(const ImageDesc* descs, uint8_t* out, int B, int S, hipStream_t s, bool antialias) {
  if (B <= 0) return;
  if (S <= 0 || S % 4 != 0) throw std::invalid_argument("resize_u8_ragged: S must be a positive multiple of 4");
  if (!descs || !out || ((uintptr_t)out & 3)) throw std::invalid_argument("resize_u8_ragged: null / misaligned operand");
  if (antialias) {
    if (B > 65535) throw std::invalid_argument("resize_u8_ragged: more than 65535 images in one antialiased launch");
    hipLaunchKernelGGL(resize_ragged_aa_kernel, dim3((S + kAaCols - 1) / kAaCols, (S + kAaRows - 1) / kAaRows, B),
                       dim3(kAaCols), 0, s, descs, out, S);
    DMLC_HIP_CHECK(hipGetLastError());
    return;
  }
  const int quads = S * S / 4;
  hipLaunchKernelGGL(resize_ragged_kernel, dim3((quads + 255) / 256, B), dim3(256), 0, s, descs, out, S);
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
