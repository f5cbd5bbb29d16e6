// Baseline (sequential Huffman) JPEG decoder -> RGB u8 HWC.
//
// Reference: the member decodes each query image with tch's
// `imagenet::load_image_and_resize` (src/services.rs:492), which uses
// libtorch-side image loading. This image has no libjpeg headers and no
// torchvision, so the node decodes with this self-contained decoder; every
// image of the reference's test_files/imagenet_1k set is baseline JPEG
// (981 YCbCr + 19 grayscale). Progressive / arithmetic-coded files are
// rejected with an error.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace dmlc {

struct Image {
  int width = 0, height = 0;
  std::vector<uint8_t> rgb;  // HWC, 3 channels
};

// Throws std::runtime_error on malformed / unsupported input.
Image decode_jpeg(const uint8_t* data, size_t size);
Image decode_jpeg_file(const std::string& path);
// Decodes straight into a caller-provided buffer: out(width, height) returns
// width * height * 3 writable bytes (e.g. pinned staging memory for the H2D
// copy; saves the Image vector's zero-fill and a copy per query image).
void decode_jpeg_into(const uint8_t* data, size_t size, const std::function<uint8_t*(int, int)>& out);

// The serving resize on the host: short side -> S (long = floor(S*long/short)),
// centre crop, bilinear with half-pixel centres, rounded to u8 [S, S, 3] HWC;
// an S x S image is copied. antialias = false is the two-tap rule of
// preprocess_host and resize_ragged_kernel. antialias = true stretches the
// triangle filter by max(scale, 1) per axis (torch's / PIL's antialias=True
// bilinear; same rule and fp32 arithmetic as resize_ragged_aa_kernel in
// csrc/kernels/resize.hip), with no rounding between the two axes.
std::vector<uint8_t> resize_u8_host(const Image& img, int S, bool antialias);

// ---- split decode: entropy decoding here, IDCT and colour on the GPU
// (csrc/kernels/jpeg_finish.hip).
struct JpegComp {
  int h = 1, v = 1;    // sampling factors
  int bw = 0, bh = 0;  // blocks per row / column of the MCU-padded plane
  size_t offset = 0;   // of the component's first coefficient (int16 units)
  uint16_t qt[64] = {0};  // quantisation table, natural (row-major) order
};
struct JpegLayout {
  int width = 0, height = 0, ncomp = 0, hmax = 1, vmax = 1;
  JpegComp comp[3];
  size_t total() const {  // int16 coefficients of the whole image
    size_t n = 0;
    for (int i = 0; i < ncomp; ++i) n += (size_t)comp[i].bw * comp[i].bh * 64;
    return n;
  }
};
// Same parser and entropy decoder as decode_jpeg (same inputs accepted, same
// errors), stopping before dequantisation: quantised coefficients, int16,
// natural order within a block, [bh][bw][64] per component, components back to
// back, written into the buffer alloc(total int16) returns (called once, when
// the frame header is read; e.g. pinned staging memory). The buffer is zeroed
// first, so blocks no scan reaches stay zero. A DC value outside int16 (only a
// forged stream reaches one) saturates.
JpegLayout decode_jpeg_coeffs(const uint8_t* data, size_t size, const std::function<int16_t*(size_t)>& alloc);
// True exactly for the layouts the integer colour conversion handles (1 or 3
// components, luma at full resolution, chroma subsampled by 1 or 2 per axis):
// the ones the GPU path finishes; everything else keeps the CPU decoder.
bool jpeg_gpu_supported(const JpegLayout& l);
// The decoder's colour stage on caller-supplied planes (plane i: u8
// [8 * comp[i].bh][8 * comp[i].bw]) -> rgb [height][width][3]: centred
// triangle chroma upsampling and 16.16 fixed-point YCbCr -> RGB. False (rgb
// untouched) when !jpeg_gpu_supported(l). The exact reference of the
// jpeg_planes_to_rgb kernel.
bool ycc_planes_to_rgb(const uint8_t* const* planes, const JpegLayout& l, uint8_t* rgb);
// Dequantisation table of the AAN inverse DCT: qt (natural order) with the
// AAN scale factors and the 2-D transform's 1/8 folded in, as the pixel
// decoder uses it.
void jpeg_aan_table(const uint16_t* qt, float* out);

}  // namespace dmlc
