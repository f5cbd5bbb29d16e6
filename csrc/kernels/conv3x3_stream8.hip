// conv3x3_stream8: the ResNet50 forms (stride 1 and 2, Cin == Cout) of the
// e4m3 3x3 conv and its public launcher; the kernel is
// conv3x3_stream8_kernel.h, the basic-block forms conv3x3_stream8_block.hip.
#include "conv3x3_stream8_kernel.h"

namespace dmlc {

namespace {

int g_stream8_variant = 0;

}  // namespace

void conv3x3_stream8_set_variant(int v) { g_stream8_variant = v; }

bool conv3x3_stream8_supported(int Hin, int Win, int Cin, int Cout, int stride) {
  if (Cin != Cout) return false;
  if (stride == 1)
    return (Hin == 28 && Win == 28 && Cin == 128) || (Hin == 14 && Win == 14 && Cin == 256) ||
           (Hin == 7 && Win == 7 && Cin == 512);
  // ResNet50 layer2.0 / layer3.0 / layer4.0 conv2 (the bottleneck's strided 3x3)
  if (stride == 2)
    return (Hin == 56 && Win == 56 && Cin == 128) || (Hin == 28 && Win == 28 && Cin == 256) ||
           (Hin == 14 && Win == 14 && Cin == 512);
  return false;
}

// Byte offset of the 16 weight bytes lane `lane` loads for (32-channel group
// j, K-tile t, N fragment nf, half h): the bytes are W8[32 j + perm32(16 nf +
// (lane & 15))][128 t + 32 fq + 16 (h ^ (fq & 1)) + 0..15], fq = lane >> 4
// (perm32 as in conv3x3_stream.hip: row 16 nf + r of a group holds channel
// 8 (r >> 2) + 4 nf + (r & 3)).
size_t conv3x3_stream8_frag_offset(int j, int t, int nf, int h, int lane, int KT) {
  return (((((size_t)j * KT + t) * 2 + nf) * 2 + h) * 64 + lane) * 16;
}

void conv3x3_stream8(const void* x, const void* wf, const float* alpha, const float* bias, void* y, const void* zero,
                     int B, int Hin, int Win, int Cin, int Cout, int stride, bool relu, float out_inv_scale,
                     hipStream_t s, const Stream8Block* blk) {
  if (B <= 0) return;
  const bool res = blk && blk->res, ds = blk && blk->wd;
  const bool block = res || ds || Cin != Cout;  // a basic-block form
  if (!(block ? conv3x3_stream8_block_supported(Hin, Win, Cin, Cout, stride, res, ds)
              : conv3x3_stream8_supported(Hin, Win, Cin, Cout, stride)))
    throw std::invalid_argument("conv3x3_stream8: unsupported shape");
  if (!x || !wf || !alpha || !bias || !y || !zero || (((uintptr_t)x | (uintptr_t)wf | (uintptr_t)zero) & 15) ||
      ((uintptr_t)y & 7) || !(out_inv_scale > 0.f))
    throw std::invalid_argument("conv3x3_stream8: null / misaligned operand or no output scale");
  if (x == y) throw std::invalid_argument("conv3x3_stream8: in-place not supported");
  const size_t xn = (size_t)B * Hin * Win * Cin, yn = (size_t)B * (Hin / stride) * (Win / stride) * Cout;
  if (res && (((uintptr_t)blk->res & 7) || ranges_overlap(blk->res, yn, y, yn) || ranges_overlap(blk->res, yn, x, xn)))
    throw std::invalid_argument("conv3x3_stream8: res is misaligned or overlaps x / y");
  if (ds && (!blk->alpha_d || !blk->bias_d || !blk->yd || (((uintptr_t)blk->wd) & 15) || ((uintptr_t)blk->yd & 7) ||
             !(blk->out_inv_scale_d > 0.f) || ranges_overlap(blk->yd, yn, y, yn) || ranges_overlap(blk->yd, yn, x, xn)))
    throw std::invalid_argument("conv3x3_stream8: null / misaligned downsample operand, no scale, or yd overlaps x / y");
  Stream8BlockArgs a;  // (the forms below launch with its Stream8Args base)
  a.x = (const uint8_t*)x;
  a.wf = (const uint8_t*)wf;
  a.alpha = alpha;
  a.bias = bias;
  a.y = (uint8_t*)y;
  a.zero = (const uint8_t*)zero;
  a.B = B;
  a.relu = relu;
  a.out_inv_scale = out_inv_scale;
  a.stagger = kernel_stagger(kStagStream8);
  if (block) {
    if (res) {
      a.res = (const uint8_t*)blk->res;
      a.res_scale = blk->res_scale;
    }
    if (ds) {
      a.wd = (const uint8_t*)blk->wd;
      a.alpha_d = blk->alpha_d;
      a.bias_d = blk->bias_d;
      a.yd = (uint8_t*)blk->yd;
      a.out_inv_scale_d = blk->out_inv_scale_d;
    }
    conv3x3_stream8_block_launch(a, Cin, stride, s);
    DMLC_HIP_CHECK(hipGetLastError());
    return;
  }
  const int v = g_stream8_variant;
  if (stride == 2 && Cin == 128) {
    // layer2.0.conv2 (56x56x128 -> 28x28): 4 output rows (9 staged rows of
    // 128-B pixels = 63 KB; 104 VGPRs: two workgroups per CU, one's staging
    // under the other's MFMAs) x all 128 channels, 4 pixel quarters x 2 groups
    // of 64. Variant 4: 7-row strips (105 KB, 164 VGPRs, one per CU):
    // 1927 vs 1923 us per resnet50_fp8 b256 forward (profiles/r5_stream8_layer2.txt)
    if (v & 4)
      launch8<28, 28, 128, 128, 7, 1, 1, 4, 2, 2, 2>(a, s);
    else
      launch8<28, 28, 128, 128, 4, 1, 1, 4, 2, 2, 2>(a, s);
  } else if (stride == 2 && Cin == 256) {
    // layer3.0.conv2 (28x28x256 -> 14x14): half an image (7 output rows, 15
    // staged rows = 105 KB) x all 256 channels, 8 groups of 32
    launch8<14, 14, 256, 256, 7, 1, 1, 1, 1, 2, 2>(a, s);
  } else if (stride == 2) {
    // layer4.0.conv2 (14x14x512 -> 7x7): one image (98 KB) x half the channels
    launch8<7, 7, 512, 512, 7, 1, 2, 1, 1, 2, 2>(a, s);
  } else if (Cin == 128) {
    // layer2 (28x28x128): half an image (14 output rows + a halo row, 54 KB)
    // x all 128 channels, 4 pixel quarters x 2 groups of 64 (the whole image,
    // 100 KB, per workgroup would stage it once per channel half)
    // (4-row strips, 108 VGPRs, two workgroups per CU: 1955 vs 1927 us per
    // resnet50_fp8 b256 forward, profiles/r5_stream8_layer2.txt)
    launch8<28, 28, 128, 128, 14, 1, 1, 4, 2, 2, 1>(a, s);
  } else if (Cin == 256) {
    // layer3: one image x half the channels per workgroup (2 pixel halves x 4
    // groups of 32; 188 VGPRs). All 256 channels per workgroup (4 groups of
    // 64 per wave) spills at any ring depth.
    launch8<14, 14, 256, 256, 14, 1, 2, 2, 1, 2, 1>(a, s);
  } else {  // layer4: two images x half the channels, 8 groups of 32
    launch8<7, 7, 512, 512, 7, 2, 2, 1, 1, 4, 1>(a, s);
  }
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
