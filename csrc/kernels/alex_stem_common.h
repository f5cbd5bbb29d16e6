// What alex_stem.hip (one workgroup per image) and alex_stem_rows.hip (one
// workgroup per pooled output row) share: the stem's geometry, the u8 ->
// paired-chunk conversion and the conv tile's swizzle. One copy, so the two
// kernels produce the same bits.
#pragma once
#include "common.h"

namespace dmlc {
namespace alex {

typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));

constexpr int kS = 224;         // input image size
constexpr int kHo = 55;         // conv output size
constexpr int kPH = 27;         // pooled output size
constexpr int kC = 64;          // output channels
constexpr int kChunks = 114;    // paired chunks per padded row (228 padded pixels)
constexpr int kRowB = 136 * 16; // staged paired row: chunks >= 114 stay zero (fragment padding reads up to 131)
constexpr int kKS = 17;         // K steps of 32 (68 chunks, 66 used)
constexpr int kU8B = kS * 3;    // 672 bytes per raw image row
constexpr int kU8Slot = 704;    // raw row slot (16-B aligned)
constexpr int kConvB = kHo * 128;  // one conv row [55][64] bf16

// conv-row byte offset of 16-B channel chunk c of pixel px
__device__ __forceinline__ int conv_off(int px, int c) { return px * 128 + ((c ^ (px & 7)) << 4); }

// Paired chunk p of padded row pr (image row pr - 2, columns 2p-2, 2p-1 =
// bytes 6p-6 .. 6p-1 of slot pr % U8RING of the raw rows) -> slot pr % RING
// (a power of two) of the paired rows: the exact values preprocess_u8 would
// produce (imagenet_norm). Branch-free: two dword
// reads issued together (a byte read per value, each under its own branch and
// wait, was most of alex_stem's time), the bytes picked by shifts, out-of-image
// values selected to zero.
template <int U8RING, int RING>
__device__ __forceinline__ void convert_chunk(const char* raw, char* ring, int pr, int p) {
  const int iy = pr - 2;
  const bool row_in = iy >= 0 && iy < kS;
  const int pc = p < 1 ? 1 : p > kChunks - 2 ? kChunks - 2 : p;  // in-row address for the edge chunks
  const int start = 6 * pc - 6;                                  // byte offset, even
  const uint32_t* src = (const uint32_t*)(raw + (pr % U8RING) * kU8Slot + (start & ~3));
  const uint32_t d0 = src[0], d1 = src[1], d2 = src[2];
  // 64-bit window starting at the first wanted byte
  const uint64_t w = (start & 2) ? ((uint64_t)d2 << 48 | (uint64_t)d1 << 16 | (d0 >> 16))
                                 : ((uint64_t)d1 << 32 | d0);
  float v[8];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int ix = 2 * p - 2 + q;
    const bool in = row_in && ix >= 0 && ix < kS;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float raw_v = (float)(uint32_t)((w >> (8 * (3 * q + c))) & 0xffu);
      v[3 * q + c] = in ? imagenet_norm(c, raw_v) : 0.f;
    }
  }
  v[6] = v[7] = 0.f;
  *(uint4*)(ring + (pr & (RING - 1)) * kRowB + p * 16) = pack8(v);
}

}  // namespace alex
}  // namespace dmlc
