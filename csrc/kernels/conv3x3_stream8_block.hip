// conv3x3_stream8's basic-block forms (ResNet18 / 34 layers 3-4 in e4m3,
// resnet18_fp8 / resnet34_fp8): the instantiations of
// conv3x3_stream8_kernel.h that a BasicBlock needs beyond a bottleneck's
// middle conv.
//
// Reference equivalent: BasicBlock.conv2 + bn2 + residual add + relu, and
// BasicBlock.conv1 + bn1 + relu with the block's downsample (1x1/s2 conv +
// bn), of tch::vision::resnet18 / resnet34.
//
//  * RES, stride 1, 14x14x256 and 7x7x512: the workgroup shapes of the
//    no-residual forms (one image x half the channels; two images x half the
//    channels), the residual's 8 bytes per store prefetched under the last
//    K-tiles: 14 more VGPRs per lane;
//  * WIDE, 14x14x256 -> 7x7x512 at stride 2: IMG = 2 images (98 KB staged)
//    x half the 512 channels per workgroup, 8 waves x 32 channels, all 7
//    pixel fragments per wave (98 of 112 MFMA rows are real pixels; one
//    image, 49 of 64). KT = 18, a ring of 2;
//  * DS: the same launch then runs the 1x1/s2 downsample over the resident
//    images' centre taps (2 K-tiles, 1/9 more MFMAs) into yd.
//
// Compiled without packed fp32 VALU ops (tools/build.py): the epilogues'
// two-channel fmas are two v_fma_f32 each here.
#include "conv3x3_stream8_kernel.h"

namespace dmlc {

bool conv3x3_stream8_block_supported(int Hin, int Win, int Cin, int Cout, int stride, bool res, bool ds) {
  if (stride == 1)
    return !ds && Cin == Cout && ((Hin == 14 && Win == 14 && Cin == 256) || (Hin == 7 && Win == 7 && Cin == 512));
  return stride == 2 && !res && Hin == 14 && Win == 14 && Cin == 256 && Cout == 512;
}

void conv3x3_stream8_block_launch(const Stream8BlockArgs& a, int Cin, int stride, hipStream_t s) {
  if (stride == 2) {  // layer4.0.conv1 (+ layer4.0.downsample)
    launch8<7, 7, 256, 512, 7, 2, 2, 1, 1, 2, 2, false, true>(a, s);
  } else if (Cin == 256) {  // layer3's conv2 (without a residual: conv3x3_stream8.hip's form)
    launch8<14, 14, 256, 256, 14, 1, 2, 2, 1, 2, 1, true>(a, s);
  } else {  // layer4's
    launch8<7, 7, 512, 512, 7, 2, 2, 1, 1, 4, 1, true>(a, s);
  }
}

}  // namespace dmlc
