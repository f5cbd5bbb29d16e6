// Glue between the host half (jpeg.h: JpegLayout) and the GPU half
// (kernels.h: JpegGpuImage) of the split JPEG decode, shared by the executor
// and the Python bindings.
#pragma once
#include <stdexcept>

#include "../kernels/kernels.h"
#include "jpeg.h"

namespace dmlc {

// Bytes of plane scratch the image needs (planes back to back).
inline size_t jpeg_plane_bytes(const JpegLayout& l) {
  size_t n = 0;
  for (int c = 0; c < l.ncomp; ++c) n += (size_t)l.comp[c].bw * l.comp[c].bh * 64;
  return n;
}

// The descriptor of an image whose coefficients start at coef_base (int16
// units) of the coefficient buffer, whose planes start at plane_base of the
// scratch buffer and whose tables are qf[table_base ..]. The layout must be
// jpeg_gpu_supported.
inline JpegGpuImage jpeg_gpu_image(const JpegLayout& l, uint8_t* rgb, size_t coef_base, size_t plane_base,
                                   int table_base) {
  if (!jpeg_gpu_supported(l)) throw std::invalid_argument("jpeg_gpu_image: layout not supported on the GPU");
  JpegGpuImage d{};
  d.rgb = rgb;
  d.width = l.width;
  d.height = l.height;
  d.ncomp = l.ncomp;
  size_t po = plane_base;
  for (int c = 0; c < l.ncomp; ++c) {
    d.hf[c] = l.hmax / l.comp[c].h;
    d.vf[c] = l.vmax / l.comp[c].v;
    d.bw[c] = l.comp[c].bw;
    d.bh[c] = l.comp[c].bh;
    d.qt[c] = table_base + c;
    d.coef_off[c] = (long long)(coef_base + l.comp[c].offset);
    d.plane_off[c] = (long long)po;
    po += (size_t)l.comp[c].bw * l.comp[c].bh * 64;
  }
  return d;
}

// The image's ncomp dequantisation tables, 64 floats each, into out.
inline void jpeg_gpu_tables(const JpegLayout& l, float* out) {
  for (int c = 0; c < l.ncomp; ++c) jpeg_aan_table(l.comp[c].qt, out + 64 * c);
}

}  // namespace dmlc
