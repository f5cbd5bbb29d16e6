// AlexNet's fused stem at query batches: u8 image -> ImageNet normalisation ->
// conv 11x11/s4/p2 (+bias) -> ReLU -> maxpool 3x3/s2, one workgroup per POOLED
// OUTPUT ROW. [B, 224, 224, 3] u8 in, [B, 27, 27, 64] bf16 NHWC out.
//
// Reference equivalent: tch::vision::alexnet's features.0-2 after
// imagenet::load_image_and_resize's normalisation, run for ONE image per query
// by `forward_t` (src/services.rs:492-493). alex_stem.hip walks an image's 55
// conv rows in one workgroup through three rings: at B = 1 that is one CU of
// the GPU for the longest launch of the forward. Here grid = (27 pooled rows,
// B), no ring and no wave roles:
//
//  * pooled row r is the 3x3/s2 max of conv rows 2r .. 2r+2, which read padded
//    image rows 8r .. 8r+18 (11 kernel rows at stride 4): the workgroup DMAs
//    those 19 raw rows (672 B each, the ones inside the image) into LDS and
//    converts them to paired-chunk rows with alex_stem's own arithmetic
//    (alex_stem_common.h). Neighbouring workgroups convert 11 of the 19 rows
//    twice: at these batches nothing waits for VALU;
//  * 8 waves as in alex_stem: pixel fragment w & 3 x channel half w >> 2, the
//    17 x 2 weight fragments in registers, loaded under the image DMA. A wave
//    runs the 3 conv rows in alex_stem's K-step order, adds the bias after the
//    MFMAs, applies ReLU and writes bf16 into a 3-row conv tile (conv_off);
//  * one barrier, then the pooled row is taken and stored as in alex_stem.
//
// Every output is the same sequence of operations as in alex_stem: the result
// is bit for bit alex_stem_u8's (tests/test_alex_stem_rows_gpu.py).
#include "alex_stem_common.h"
#include "kernels.h"

namespace dmlc {

namespace {

using namespace alex;

constexpr int kRows = 19;   // padded image rows of one pooled row: 8r .. 8r + 18
constexpr int kSlots = 32;  // ... in slot pr % 32 of the raw and paired rows (convert_chunk's addressing)
constexpr size_t kLds = (size_t)kSlots * kRowB + 3 * (size_t)kConvB + (size_t)kSlots * kU8Slot;

struct StemRowsArgs {
  const uint8_t* x;   // [B, 224, 224, 3]
  const bf16* w;      // [64][544] paired-chunk K order (alex_stem_k)
  const float* bias;  // [64]
  bf16* y;            // [B, 27, 27, 64]
};

__global__ __launch_bounds__(512, 1) void alex_stem_rows_kernel(StemRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  char* pair = (char*)smem;             // [32][kRowB] paired rows
  char* conv = pair + kSlots * kRowB;   // [3][55][64] bf16 conv rows
  char* raw = conv + 3 * kConvB;        // [32][kU8Slot] raw image rows
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int r = blockIdx.x, b = blockIdx.y;
  const uint8_t* img = a.x + (long)b * kS * kU8B;

  // raw rows of padded rows 8r + i (image row 8r + i - 2), one row per wave and turn
  for (int i = wave; i < kRows; i += 8) {
    const int iy = 8 * r + i - 2;
    if (iy >= 0 && iy < kS && lane < kU8B / 16)
      dma16(img + (long)iy * kU8B + lane * 16, raw + ((8 * r + i) % kSlots) * kU8Slot);
  }
  // the fragment-padding chunks (>= 114) must read as finite zeros (they meet zero weights)
  for (int o = tid * 16; o < kSlots * kRowB; o += 512 * 16) *(uint4*)(pair + o) = make_uint4(0, 0, 0, 0);

  // weights: wave's channel group 32 (w >> 2), n-blocks nf = 0, 1 (rows permuted)
  const int ch0 = 32 * (wave >> 2);
  bf16x8 wr[kKS][2];
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
    const bf16* row = a.w + (long)(ch0 + perm32(16 * nf + fr)) * (kKS * 32);
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) wr[ks][nf] = *(const bf16x8*)(row + ks * 32 + fq * 8);
  }
  float bs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bs[e] = a.bias[ch0 + 8 * fq + e];

  // per-lane B-operand constants: chunk c = 4 ks + fq = (kh, cc); kh = 11
  // (the two pad chunks) reads row 10 (finite values x zero weights)
  const int ow = 16 * (wave & 3) + fr;
  int kh_of[kKS], col_of[kKS];
#pragma unroll
  for (int ks = 0; ks < kKS; ++ks) {
    const int c = 4 * ks + fq;
    const int kh = c / 6, cc = c - 6 * (c / 6);
    kh_of[ks] = kh < 11 ? kh : 10;
    col_of[ks] = (2 * ow + cc) * 16;
  }

  vm_wait<0>();  // the raw rows (and the weights) have landed
  lgkm_wait();
  __syncthreads();
  for (int it = tid; it < kRows * kChunks; it += 512) {
    const int i = it / kChunks, p = it - i * kChunks;
    convert_chunk<kSlots, kSlots>(raw, pair, 8 * r + i, p);
  }
  lgkm_wait();
  __syncthreads();

  // ---- conv rows 2r + rr (padded rows 8r + 4rr + kh): 17 k-steps x 2 n-blocks each
#pragma unroll
  for (int rr = 0; rr < 3; ++rr) {
    floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
    bf16x8 xb[kKS];
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks)
      xb[ks] = *(const bf16x8*)(pair + ((8 * r + 4 * rr + kh_of[ks]) & (kSlots - 1)) * kRowB + col_of[ks]);
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[ks][0], xb[ks], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[ks][1], xb[ks], acc[1], 0, 0, 0);
    }
    // lane: channels ch0 + 8 fq .. +7 of pixel ow (nf 0: +0..3, nf 1: +4..7)
    if (ow < kHo) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = acc[0][e] + bs[e];
        v[4 + e] = acc[1][e] + bs[4 + e];
      }
      *(uint4*)(conv + rr * kConvB + conv_off(ow, ch0 / 8 + fq)) = relu_bf16x8(pack8(v));
    }
  }
  lgkm_wait();
  __syncthreads();

  // ---- pooled row r (post-ReLU values are >= 0: bf16 max = unsigned 16-bit max)
  if (tid < kPH * 8) {
    const int pw = tid >> 3, cg = tid & 7;
    ushort8 m = ushort8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx)
        m = __builtin_elementwise_max(m, *(const ushort8*)(conv + dy * kConvB + conv_off(2 * pw + dx, cg)));
    *(ushort8*)(a.y + (((long)b * kPH + r) * kPH + pw) * kC + cg * 8) = m;
  }
}

}  // namespace

void alex_stem_rows_u8(const uint8_t* x, const void* w, const float* bias, void* y, int B, hipStream_t s) {
  if (B <= 0) return;
  if (!x || !w || !bias || !y || ((uintptr_t)x & 15) || ((uintptr_t)w & 15) || ((uintptr_t)y & 15))
    throw std::invalid_argument("alex_stem_rows_u8: null / misaligned operand");
  if (B > 65535) throw std::invalid_argument("alex_stem_rows_u8: batch too large");
  const StemRowsArgs a{x, (const bf16*)w, bias, (bf16*)y};
  hipLaunchKernelGGL(alex_stem_rows_kernel, dim3(kPH, B), dim3(512), kLds, s, a);
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
