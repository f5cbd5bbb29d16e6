// The GPU half of the split JPEG decode: the host stops after entropy
// decoding (decode_jpeg_coeffs, csrc/runtime/jpeg.cpp) and uploads quantised
// coefficients; two launches over a ragged batch finish the images.
//
// Stage 1, jpeg_idct_planes: per 8x8 block, dequantise with the component's
// table (AAN scale factors folded in on the host), 2-D inverse DCT in fp32 on
// the AAN flowgraph of the host decoder (columns first, like it), + 128,
// round half up, clamp -> the component's padded u8 plane in scratch. 8 lanes
// per block, 8 blocks per wave, 32 per workgroup: lane j loads row j of the
// block as one 16-B vector (a wave reads 1 KB contiguous), the block goes
// through an LDS tile for the column pass and again for the row pass, and
// lane j stores the 8 bytes of pixel row j. Grid = (block chunks of the
// largest plane, 3 x images); a (image, component) pair with fewer blocks
// leaves its surplus workgroups at once.
//
// Stage 2, jpeg_planes_to_rgb: per output pixel, the centred 3:1 triangle
// chroma upsampling and the 16.16 fixed-point YCbCr -> RGB of the host
// decoder (chroma_row / ycc_pixel), in the same integer arithmetic, so the
// result is bit-identical to ycc_planes_to_rgb on the same planes. One thread
// writes 4 consecutive pixels = 12 B as three dword stores (resize.hip's
// scheme); grid = (pixel blocks of the largest image, images).
//
// Every index comes from the descriptors, which the launchers validate on the
// host against the buffer sizes: coefficient VALUES never reach an address.
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace dmlc {

namespace {

constexpr int kIdctBlocks = 32;  // 8x8 blocks per workgroup (8 lanes each)

// One 8-point AAN inverse DCT (the host's DMLC_IDCT8_LANES, scalar).
__device__ inline void idct8(const float* in, float* o) {
  const float t10 = in[0] + in[4], t11 = in[0] - in[4];
  const float t13 = in[2] + in[6], t12 = (in[2] - in[6]) * 1.414213562f - t13;
  const float e0 = t10 + t13, e3 = t10 - t13, e1 = t11 + t12, e2 = t11 - t12;
  const float z13 = in[5] + in[3], z10 = in[5] - in[3];
  const float z11 = in[1] + in[7], z12 = in[1] - in[7];
  const float o7 = z11 + z13;
  const float t11b = (z11 - z13) * 1.414213562f;
  const float z5 = (z10 + z12) * 1.847759065f;
  const float t10b = z12 * 1.082392200f - z5;
  const float t12b = z10 * -2.613125930f + z5;
  const float o6 = t12b - o7;
  const float o5 = t11b - o6;
  const float o4 = t10b + o5;
  o[0] = e0 + o7;
  o[7] = e0 - o7;
  o[1] = e1 + o6;
  o[6] = e1 - o6;
  o[2] = e2 + o5;
  o[5] = e2 - o5;
  o[4] = e3 + o4;
  o[3] = e3 - o4;
}

__global__ __launch_bounds__(kIdctBlocks * 8) void jpeg_idct_kernel(const JpegGpuImage* __restrict__ descs,
                                                                    const float* __restrict__ qf,
                                                                    const int16_t* __restrict__ coef,
                                                                    uint8_t* __restrict__ planes) {
  const int img = blockIdx.y / 3, c = blockIdx.y % 3;
  const JpegGpuImage* d = descs + img;
  if (c >= d->ncomp) return;  // (uniform over the workgroup, like the next return)
  const int bw = d->bw[c], nblk = bw * d->bh[c];
  const int b0 = blockIdx.x * kIdctBlocks;
  if (b0 >= nblk) return;
  const int lb = threadIdx.x >> 3, j = threadIdx.x & 7;
  const int b = b0 + lb;
  const bool valid = b < nblk;
  // [block][row][column], rows padded to 9 floats
  __shared__ float tile[kIdctBlocks][8][9];
  float x[8], o[8];
  if (valid) {
    const int4 raw = *(const int4*)(coef + d->coef_off[c] + (long long)b * 64 + j * 8);
    const float4* q = (const float4*)(qf + (long long)d->qt[c] * 64 + j * 8);
    const float4 q0 = q[0], q1 = q[1];
    x[0] = (float)(short)(raw.x & 0xffff) * q0.x;
    x[1] = (float)(raw.x >> 16) * q0.y;
    x[2] = (float)(short)(raw.y & 0xffff) * q0.z;
    x[3] = (float)(raw.y >> 16) * q0.w;
    x[4] = (float)(short)(raw.z & 0xffff) * q1.x;
    x[5] = (float)(raw.z >> 16) * q1.y;
    x[6] = (float)(short)(raw.w & 0xffff) * q1.z;
    x[7] = (float)(raw.w >> 16) * q1.w;
  } else {
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = 0.f;
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) tile[lb][j][u] = x[u];
  __syncthreads();
  // pass 1: lane j owns column j (frequency u = j), transforms over v
#pragma unroll
  for (int v = 0; v < 8; ++v) x[v] = tile[lb][v][j];
  idct8(x, o);
#pragma unroll
  for (int y = 0; y < 8; ++y) tile[lb][y][j] = o[y];  // (its own column: no other lane reads or writes it)
  __syncthreads();
  // pass 2: lane j owns pixel row j, transforms over u
#pragma unroll
  for (int u = 0; u < 8; ++u) x[u] = tile[lb][j][u];
  idct8(x, o);
  uint32_t w[2] = {0, 0};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // round half up; negatives clamp to 0 (the host's idct8x8_generic)
    const float f = fminf(fmaxf(o[k] + 128.5f, 0.f), 255.f);
    w[k >> 2] |= (uint32_t)(int)f << (8 * (k & 3));
  }
  if (valid) {
    const int by = b / bw, bx = b - by * bw;
    uint8_t* dst = planes + d->plane_off[c] + ((long long)(by * 8 + j) * bw + bx) * 8;
    *(uint2*)dst = make_uint2(w[0], w[1]);
  }
}

// The chroma sample at output pixel (x, y): chroma_row's arithmetic.
__device__ inline int chroma_at(const uint8_t* __restrict__ pl, int pw, int cw, int ch, int hf, int vf, int x, int y) {
  int y0 = y, y1 = y, wa = 4, wb = 0;  // weights of rows y0, y1 (sum 4)
  if (vf == 2) {
    y0 = y >> 1;
    y1 = (y & 1) ? min(y0 + 1, ch - 1) : max(y0 - 1, 0);
    wa = 3;
    wb = 1;
  }
  const uint8_t* r0 = pl + (long long)y0 * pw;
  const uint8_t* r1 = pl + (long long)y1 * pw;
  if (hf == 1) return (wa * r0[x] + wb * r1[x] + 2) >> 2;
  const int i = x >> 1;
  const int nb = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);
  const int ti = wa * r0[i] + wb * r1[i], tn = wa * r0[nb] + wb * r1[nb];
  return (3 * ti + tn + 8) >> 4;
}

// JFIF full-range constants, 16.16 (the host's kCrR, kCbG, kCrG, kCbB)
constexpr int kCrR = 91881, kCbB = 116130, kCrG = -46802, kCbG = -22554;

__device__ inline int clamp_fix(int v) {  // 16.16 -> u8, rounded
  v = (v + 32768) >> 16;
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const JpegGpuImage* __restrict__ descs,
                                                       const uint8_t* __restrict__ planes) {
  const JpegGpuImage* d = descs + blockIdx.y;
  const int W = d->width, H = d->height;
  const int npx = W * H;  // <= 2^28 (validated)
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= npx) return;
  const bool colour = d->ncomp == 3;
  const uint8_t* py = planes + d->plane_off[0];
  const int pw = d->bw[0] * 8;
  const uint8_t *pb = nullptr, *pr = nullptr;
  int pwb = 0, pwr = 0, cwb = 0, chb = 0, cwr = 0, chr = 0, hfb = 1, vfb = 1, hfr = 1, vfr = 1;
  if (colour) {
    pb = planes + d->plane_off[1];
    pr = planes + d->plane_off[2];
    pwb = d->bw[1] * 8;
    pwr = d->bw[2] * 8;
    hfb = d->hf[1], vfb = d->vf[1], hfr = d->hf[2], vfr = d->vf[2];
    cwb = (W + hfb - 1) / hfb, chb = (H + vfb - 1) / vfb;  // the valid chroma area
    cwr = (W + hfr - 1) / hfr, chr = (H + vfr - 1) / vfr;
  }
  uint8_t v[12];
  const int n = min(4, npx - p0);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = min(p0 + k, npx - 1);
    const int y = p / W, x = p - y * W;
    const int Yv = py[(long long)y * pw + x];
    if (colour) {
      const int cb = chroma_at(pb, pwb, cwb, chb, hfb, vfb, x, y) - 128;
      const int cr = chroma_at(pr, pwr, cwr, chr, hfr, vfr, x, y) - 128;
      const int Y = Yv << 16;
      v[3 * k] = (uint8_t)clamp_fix(Y + kCrR * cr);
      v[3 * k + 1] = (uint8_t)clamp_fix(Y + kCbG * cb + kCrG * cr);
      v[3 * k + 2] = (uint8_t)clamp_fix(Y + kCbB * cb);
    } else {
      v[3 * k] = v[3 * k + 1] = v[3 * k + 2] = (uint8_t)Yv;
    }
  }
  uint8_t* dst = d->rgb + (long long)p0 * 3;
  if (n == 4) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
      ((uint32_t*)dst)[i] = (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) | ((uint32_t)v[4 * i + 2] << 16) |
                            ((uint32_t)v[4 * i + 3] << 24);
  } else {  // the image's last 1-3 pixels
#pragma unroll
    for (int i = 0; i < 9; ++i)
      if (i < 3 * n) dst[i] = v[i];
  }
}

// Everything a kernel derives an address from, against the buffer sizes.
// idct: the coefficient side too (stage 1); rgb: the destination (stage 2).
void check_images(const char* who, const JpegGpuImage* host, int n, int n_tables, size_t coef_elems,
                  size_t plane_bytes, bool idct, bool rgb) {
  auto bad = [&](int i, const char* what) {
    throw std::invalid_argument(std::string(who) + ": image " + std::to_string(i) + ": " + what);
  };
  for (int i = 0; i < n; ++i) {
    const JpegGpuImage& d = host[i];
    if (d.ncomp != 1 && d.ncomp != 3) bad(i, "component count");
    if (d.width < 1 || d.height < 1 || d.width > 16384 || d.height > 16384) bad(i, "size");
    for (int c = 0; c < d.ncomp; ++c) {
      const int hf = d.hf[c], vf = d.vf[c];
      if (c == 0 ? (hf != 1 || vf != 1) : (hf < 1 || hf > 2 || vf < 1 || vf > 2)) bad(i, "sampling");
      if (d.bw[c] < 1 || d.bh[c] < 1 || d.bw[c] > 4096 || d.bh[c] > 4096) bad(i, "block counts");
      // the area the colour stage reads lies inside the plane
      if ((d.width + hf - 1) / hf > 8 * d.bw[c] || (d.height + vf - 1) / vf > 8 * d.bh[c]) bad(i, "plane smaller than image");
      const unsigned long long blocks = (unsigned long long)d.bw[c] * d.bh[c];
      if (d.plane_off[c] < 0 || (d.plane_off[c] & 7) || (unsigned long long)d.plane_off[c] + blocks * 64 > plane_bytes)
        bad(i, "plane outside the scratch buffer");
      if (idct) {
        if (d.coef_off[c] < 0 || (d.coef_off[c] & 7) || (unsigned long long)d.coef_off[c] + blocks * 64 > coef_elems)
          bad(i, "coefficients outside the buffer");
        if (d.qt[c] < 0 || d.qt[c] >= n_tables) bad(i, "table index");
      }
    }
    if (rgb && (!d.rgb || ((uintptr_t)d.rgb & 3))) bad(i, "null / misaligned destination");
  }
}

}  // namespace

void jpeg_idct_planes(const JpegGpuImage* host, const JpegGpuImage* dev, int n, const float* qf, int n_tables,
                      const int16_t* coef, size_t coef_elems, uint8_t* planes, size_t plane_bytes, hipStream_t s) {
  if (n <= 0) return;
  if (n > 21845) throw std::invalid_argument("jpeg_idct_planes: more than 21845 images");  // grid.y = 3 n
  if (!host || !dev || !qf || !coef || !planes || ((uintptr_t)qf & 15) || ((uintptr_t)coef & 15) ||
      ((uintptr_t)planes & 7))
    throw std::invalid_argument("jpeg_idct_planes: null / misaligned operand");
  check_images("jpeg_idct_planes", host, n, n_tables, coef_elems, plane_bytes, true, false);
  int most = 0;
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < host[i].ncomp; ++c) most = std::max(most, host[i].bw[c] * host[i].bh[c]);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((most + kIdctBlocks - 1) / kIdctBlocks, 3 * n), dim3(kIdctBlocks * 8), 0,
                     s, dev, qf, coef, planes);
  DMLC_HIP_CHECK(hipGetLastError());
}

void jpeg_planes_to_rgb(const JpegGpuImage* host, const JpegGpuImage* dev, int n, const uint8_t* planes,
                        size_t plane_bytes, hipStream_t s) {
  if (n <= 0) return;
  if (n > 65535) throw std::invalid_argument("jpeg_planes_to_rgb: more than 65535 images");
  if (!host || !dev || !planes) throw std::invalid_argument("jpeg_planes_to_rgb: null operand");
  check_images("jpeg_planes_to_rgb", host, n, 0, 0, plane_bytes, false, true);
  long long most = 0;
  for (int i = 0; i < n; ++i) most = std::max(most, (long long)host[i].width * host[i].height);
  hipLaunchKernelGGL(jpeg_rgb_kernel, dim3((unsigned)((most + 1023) / 1024), n), dim3(256), 0, s, dev, planes);
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
