// Stride-2 3x3 conv 56x56xCI -> 28x28x128 (BN folded, ReLU), row-streamed, in
// two shapes of one template:
//  * CI = 64 (S2Shape64): ResNet18 layer2.0.conv1, optionally together with the
//    block's 1x1/s2 downsample (BN folded, no ReLU; DS);
//  * CI = 128 (S2Shape128): ResNet50 layer2.0.conv2, the first layer2
//    bottleneck's strided 3x3, with a bf16 or an e4m3 output (OUT8:
//    relu(v) * out_inv_scale, saturated, for ResNet50's e4m3 expand conv,
//    EngineOptions::fp8_3x3_out).
//
// Reference equivalent: layer2.0.{conv1,bn1,relu} and layer2.0.downsample of
// tch::vision::resnet18, layer2.0.{conv2,bn2,relu} of tch::vision::resnet50
// (src/services.rs:513-524 loads them; `forward_t` runs them per query,
// src/services.rs:493). As a stream conv (conv3x3_stream.hip: strips of
// output rows with their input rows resident in LDS) the input staging of
// every round of workgroups is exposed: 72 us for 33 GFLOP at CI = 64
// (profiles/r2_final_resnet18_kernels.txt), 102 us at CI = 128
// (profiles/r4_r50_3x3_e4m3_out.txt), both at B = 256. Here one workgroup
// walks one image top to bottom (one round at B = 256), R output rows per
// step, the 2R input rows of the next step arriving by LDS-DMA while the
// current step computes:
//
//  * weight-stationary: 4 waves (one per SIMD), wave w owns output channels
//    32w .. 32w + 31 and keeps all their K-step fragments in registers (CI =
//    64: 18 for the 3x3 taps + 2 for the downsample; CI = 128: 36, 288 VGPRs
//    of the 512-register budget of a single wave per SIMD), so the only
//    global traffic in the loop is the row DMA (whose vmcnt, being asm, the
//    compiler cannot see or wait on) and the output stores;
//  * R = 4 output rows per step at CI = 64 (112 pixels = 7 fragments); R = 2
//    at CI = 128 (56 pixels = 3.5 fragments: the 4th fragment's last 8 lanes
//    re-read pixel 55 and store nothing), where 4 rows would need a 17-row
//    ring of 14.6 KB rows;
//  * staged input row: CI / 32 planes (32 channels each) of 57 pixel slots x
//    64 B (slot 0 = column -1, zero; 1..28 = odd columns; 29..56 = even
//    columns), so output pixels c, c+1 read adjacent slots at every tap (kw 0:
//    slot c, kw 1: 29 + c as an immediate, kw 2: c + 1); rows are a bank-row
//    multiple (CI = 64: planes padded to 58 slots, 7424 B rows; CI = 128:
//    14592 B = 57 x 256) in a ring of 4R + 1 rows + 2 guard slots (copies of
//    slots 0, 1) so the 3 kernel rows of a fragment are immediate offsets of
//    one address;
//  * 16-B chunk c of a plane of stored pixel (y, x) sits at physical chunk
//    c ^ ((K >> 1) & 3), K = ((y + 1) >> 1) * 28 + ((x + 1) >> 1): along a
//    fragment K is the output pixel index plus a tap constant, also where a
//    fragment wraps an output row, and every ds_read_b128 is conflict free
//    (tests/test_layouts_cpu.py).
#include "common.h"
#include "kernels.h"

#include <string>

namespace dmlc {

namespace {

constexpr int kHI = 56, kWI = 56, kH = 28, kW = 28, kCO = 128;
constexpr int kE0 = 29;            // first even-column slot
constexpr int kRun = 4 * 2 * kW;   // 224 DMA chunks per plane (slots 1..56)
constexpr int kOffKw1 = kE0 * 64;  // kw = 1 reads slot 29 + c
constexpr int kCT = 2;             // downsample K steps

// Ring lengths: rows 2 r0 - 1 .. 2 r0 + 2R - 1 in use + 2R in flight. Literals, because the tests' modelled
// faults read them from this file (tests/_kernel_bar.py kernel_const): kRing is the 64-channel shape's,
// under the name it has always had, kRing128 the 128-channel shape's.
constexpr int kRing = 17;
constexpr int kRing128 = 9;

struct S2Shape64 {
  static constexpr int CI = 64, R = 4, kRingRows = kRing;
  static constexpr int kPlane = 58 * 64;  // 3712 B: 7424 B rows are a bank-row multiple
  struct Args {
    const bf16* x;      // [B, 56, 56, 64]
    const bf16* wf;     // 3x3 weights, fragment order [4][18][2][64][8] (stream_frag_index, K = 576)
    const bf16* wdf;    // 1x1 weights, fragment order [4][2][2][64][8] (K = 64)
    const float* bias;  // [128]
    const float* bd;    // [128]
    bf16* y;            // [B, 28, 28, 128]
    bf16* yd;           // [B, 28, 28, 128]
    const bf16* zero;
    int relu;
    int stagger;  // start_stagger (common.h)
  };
};
struct S2Shape128 {
  static constexpr int CI = 128, R = 2, kRingRows = kRing128;
  static constexpr int kPlane = 57 * 64;  // 3648 B: 14592 B rows = 57 x 256
  struct Args {
    const bf16* x;      // [B, 56, 56, 128]
    const bf16* wf;     // weights, fragment order [4][36][2][64][8] (stream_frag_index, K = 1152)
    const float* bias;  // [128]
    void* y;            // [B, 28, 28, 128], bf16 or (out_inv_scale > 0) e4m3
    int relu;
    float out_inv_scale;
  };
};

// everything else about a shape follows from those four
template <class S>
struct S2Derived {
  static constexpr int kPlanes = S::CI / 32;       // 32-channel planes of a staged row = K steps per tap
  static constexpr int kRB = kPlanes * S::kPlane;  // bytes per staged row
  static constexpr int kSlotsAlloc = S::kRingRows + 2;
  static constexpr int kSteps = kH / S::R;
  static constexpr int kNPix = S::R * kW;        // output pixels per step
  static constexpr int kMF = (kNPix + 15) / 16;  // pixel fragments per step
  static constexpr int kKT = 9 * kPlanes;        // 3x3 K steps
  static constexpr size_t kLds = (size_t)kSlotsAlloc * kRB;
  static_assert(S::kRingRows == 4 * S::R + 1, "ring: the rows in use and the rows in flight");
  static_assert(kH % S::R == 0 && kLds <= 160 * 1024, "LDS budget");
};

__device__ __forceinline__ int swz_of(int y, int x) { return ((((y + 1) >> 1) * kW + ((x + 1) >> 1)) >> 1) & 3; }

// DS: also the block's 1x1/s2 downsample (K = 64 more, the yd output). Off
// (ds_into_conv2): the downsample is a K-extension of the block's conv2
// (conv3x3_rows28_kernel DSX), so yd is neither written here nor read back
// there: 51 of the 205 MB this kernel moved at B = 256, and 2 of its 20 K steps.
template <class S, bool DS, bool OUT8>
__global__ __launch_bounds__(256, 1) void conv3x3_s2rows_kernel(typename S::Args a) {
  using D = S2Derived<S>;
  static_assert(!DS || S::CI == 64, "the downsample form exists for 64 input channels only");
  static_assert(!OUT8 || S::CI == 128, "the e4m3 output exists for 128 input channels only");
  constexpr int kCI = S::CI, kR = S::R, kRingS = S::kRingRows, kPlane = S::kPlane, kPlanes = D::kPlanes;
  constexpr int kRB = D::kRB, kSlotsAlloc = D::kSlotsAlloc, kSteps = D::kSteps, kNPix = D::kNPix, kMF = D::kMF;
  constexpr int kKT = D::kKT, kKS = kKT + (DS ? kCT : 0);
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  char* ring = (char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the start stagger (kStagS2rows) was tuned for, and is wired to, the 64-channel form only
  if constexpr (kCI == 64) start_stagger(a.stagger);
  const int fr = lane & 15, g = lane >> 4;
  const int b = blockIdx.x;
  const bf16* img = a.x + (long)b * kHI * kWI * kCI;

  // Every slot's pad column (slot 0 of each plane), its spare slot, the
  // spare guard copies and the zero row y = -1 are zeroed once here and
  // never DMA'd over (a shared zero page read by every workgroup's pad lanes
  // is one hot L2 channel per XCD).
  for (int o = tid * 16; o < kSlotsAlloc * kRB; o += 256 * 16) *(uint4*)(ring + o) = make_uint4(0, 0, 0, 0);
  lds_barrier();
  // input row yy >= 0 -> ring slot (yy + 1) % kRingS, and guard slot kRingS /
  // kRingS + 1 too for slots 0 / 1: per plane the 224 chunks of slots 1..56 are
  // one contiguous run; wave w DMAs chunks 64 w .. 64 w + 63 of every run
  auto load_row = [&](int yy) __attribute__((always_inline)) {
    const int slot = (yy + 1) % kRingS;
    const int k = wave * 64 + lane;
    const int pos = 1 + (k >> 2), c = k & 3;
    const int x = pos < kE0 ? 2 * pos - 1 : 2 * (pos - kE0);
    const int sw = swz_of(yy, x);
    auto load_plane = [&](int q, const bf16* src, bool live) __attribute__((always_inline)) {
      char* dst = ring + q * kPlane + 64 + wave * 1024;
      if (live) {
        dma16(src, dst + slot * kRB);
        if (slot < 2) dma16(src, dst + (slot + kRingS) * kRB);
      }
    };
    // One loop, written in each shape's own form: where the k < kRun test sits and how the channel
    // offset is associated change the register allocation of the whole kernel, so both keep theirs
    if constexpr (kCI == 64) {
#pragma unroll
      for (int q = 0; q < kPlanes; ++q)
        load_plane(q, img + ((long)yy * kWI + x) * kCI + 8 * (4 * q + (c ^ sw)), k < kRun);
    } else if (k < kRun) {
#pragma unroll
      for (int q = 0; q < kPlanes; ++q)
        load_plane(q, img + ((long)yy * kWI + x) * kCI + 32 * q + 8 * (c ^ sw), true);
    }
  };
  // this lane's 8 output channels ch0 + 8g .. +7 (weight rows permuted,
  // perm32); loaded before the row DMAs so the prologue wait below can leave
  // exactly the weight loads in flight
  const int ch0 = wave * 32;
  float bs[8], bsd[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bs[e] = a.bias[ch0 + 8 * g + e];
    if constexpr (DS) bsd[e] = a.bd[ch0 + 8 * g + e];
  }
  for (int yy = 0; yy <= 2 * kR - 1; ++yy) load_row(yy);  // step 0 reads rows -1 .. 2R - 1

  // ---- per-lane constants. Fragment f covers step pixels p = 16 f + fr (row
  // p / 28 of the step, column c = p % 28). col[f][v]: the in-row byte offset
  // of plane 0 for variant v = (kw == 2) + 2 (kh == 2)
  int prow2[kMF], col[kMF][4];
#pragma unroll
  for (int f = 0; f < kMF; ++f) {
    int p = 16 * f + fr;
    // R * 28 pixels do not fill the last fragment: its lanes past the last pixel re-read it
    if constexpr (kNPix % 16 != 0) p = min(p, kNPix - 1);
    prow2[f] = 2 * (p / kW);
    const int c = p % kW;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int kw2 = v & 1, kh2 = v >> 1;
      const int s = ((p + kw2 + kW * kh2) >> 1) & 3;  // K of r0 = 0 (28 r0 = 28 R step: a multiple of 8)
      col[f][v] = (c + kw2) * 64 + ((g ^ s) << 4);
    }
  }
  bf16x8 w[kKS][2];
#pragma unroll
  for (int t = 0; t < kKS; ++t)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      const bf16* src;
      if constexpr (DS)  // (one conditional expression: as two statements the DS form allocates registers differently)
        src = t < kKT ? a.wf + ((((long)wave * kKT + t) * 2 + nf) * 64 + lane) * 8
                      : a.wdf + ((((long)wave * kCT + (t - kKT)) * 2 + nf) * 64 + lane) * 8;
      else
        src = a.wf + ((((long)wave * kKT + t) * 2 + nf) * 64 + lane) * 8;
      w[t][nf] = *(const bf16x8*)src;
    }
  // the prologue rows (DMA'd before the weights) have landed; the weights may
  // still be in flight: the first step's MFMAs wait for each K step's own
  // fragments (the compiler's counted waits), so the weight load from L2
  // overlaps the first step instead of preceding it (vmcnt tops out at 63)
  vm_wait<(2 * kKS < 63 ? 2 * kKS : 63)>();
  __builtin_amdgcn_s_barrier();

  // step 0 is peeled (a separate copy of the body): at a loop header the
  // compiler waits for every outstanding load (vmcnt(0)), which would put the
  // whole weight load back in front of the first MFMA
  auto step_body = [&](const int step) __attribute__((always_inline)) {
    const int r0 = step * kR;  // first output row; input rows 2 r0 - 1 .. 2 r0 + 2R - 1
    if (step + 1 < kSteps)
      for (int yy = 2 * r0 + 2 * kR; yy <= 2 * r0 + 4 * kR - 1; ++yy) load_row(yy);
    // ring slot of kernel row 0 of every fragment (+ kh rows: immediate, guard slots)
    const int sb = (2 * r0) % kRingS;
    int rowoff[kMF];
#pragma unroll
    for (int f = 0; f < kMF; ++f) {
      int sl = sb + prow2[f];
      sl = sl >= kRingS ? sl - kRingS : sl;
      rowoff[f] = sl * kRB;
    }
    floatx4 acc[kMF][2], accd[kMF][2];
#pragma unroll
    for (int f = 0; f < kMF; ++f)
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        // CI = 64 starts its accumulators at the bias, CI = 128 adds the bias in the epilogue: the
        // fp32 roundings differ, so either form keeps the results it has always given
        if constexpr (kCI == 64) {
          acc[f][nf] = floatx4{bs[4 * nf], bs[4 * nf + 1], bs[4 * nf + 2], bs[4 * nf + 3]};
          if constexpr (DS) accd[f][nf] = floatx4{bsd[4 * nf], bsd[4 * nf + 1], bsd[4 * nf + 2], bsd[4 * nf + 3]};
        } else {
          acc[f][nf] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
      }
    // K step t: tap = t / kPlanes (downsample steps: tap 4 = (1, 1)), plane q = t % kPlanes
    auto xread = [&](int t, int f) __attribute__((always_inline)) {
      const int tap = t < kKT ? t / kPlanes : 4, q = t % kPlanes;
      const int kh = tap / 3, kw = tap % 3;
      const int v = (kw == 2) + 2 * (kh == 2);
      const int imm = kh * kRB + (kw == 1 ? kOffKw1 : 0) + q * kPlane;
      return *(const bf16x8*)(ring + (rowoff[f] + col[f][v]) + imm);
    };
    bf16x8 xc[kMF];
#pragma unroll
    for (int f = 0; f < kMF; ++f) xc[f] = xread(0, f);
#pragma unroll
    for (int t = 0; t < kKS; ++t) {
#pragma unroll
      for (int f = 0; f < kMF; ++f) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) {
          if (t < kKT)
            acc[f][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[t][nf], xc[f], acc[f][nf], 0, 0, 0);
          else
            accd[f][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[t][nf], xc[f], accd[f][nf], 0, 0, 0);
        }
        if (t + 1 < kKS) xc[f] = xread(t + 1, f);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- epilogue: lane holds channels ch0 + 8g .. +7 of step pixel 16 f + fr
#pragma unroll
    for (int f = 0; f < kMF; ++f) {
      // The element offset: with whole fragments the step pixel enters it inline and it comes before
      // the values; a partial last fragment needs p for its store predicate, uses it in the offset and
      // computes both after the values. Either form elsewhere changes the kernel's register allocation.
      long o;
      bool live = true;
      if constexpr (kNPix % 16 == 0) o = (((long)b * kH + r0) * kW + 16 * f + fr) * kCO + ch0 + 8 * g;
      float v[8], vd[8];
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[4 * nf + i] = kCI == 64 ? acc[f][nf][i] : acc[f][nf][i] + bs[4 * nf + i];
          if constexpr (DS) vd[4 * nf + i] = accd[f][nf][i];
        }
      if constexpr (kNPix % 16 != 0) {
        const int p = 16 * f + fr;
        live = p < kNPix;  // the clamped lanes store nothing
        o = (((long)b * kH + r0) * kW + p) * kCO + ch0 + 8 * g;
      }
      if constexpr (OUT8) {  // the e4m3 output of ResNet50's fp8 path
        float qv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          qv[e] = fminf(fmaxf((a.relu ? fmaxf(v[e], 0.f) : v[e]) * a.out_inv_scale, -448.f), 448.f);
        const uint2 pk =
            make_uint2(e4m3x4_from_f32(qv[0], qv[1], qv[2], qv[3]), e4m3x4_from_f32(qv[4], qv[5], qv[6], qv[7]));
        if (live) *(uint2*)((uint8_t*)a.y + o) = pk;
      } else {
        const uint4 pk = pack8_relu(v, a.relu);
        if (live) *(uint4*)((bf16*)a.y + o) = pk;
      }
      if constexpr (DS) *(uint4*)(a.yd + o) = pack8(vd);
    }
    // the next step's rows have landed (the (2) kMF stores just issued may
    // still be in flight: vmcnt retires in order) and every wave is done
    // reading the rows they replace
    vm_wait<(DS ? 2 : 1) * kMF>();
    lds_barrier();
  };
  step_body(0);
  for (int step = 1; step < kSteps; ++step) step_body(step);
}

// The one validation and launch path of both entry points (null for an operand a shape does not have).
template <class S>
void s2rows_launch(const char* who, const typename S::Args& a, const void* wdf, const void* bd, const void* yd,
                   const void* zero, bool out8, int B, hipStream_t s) {
  if (B <= 0) return;
  auto fail = [&](const char* what) { throw std::invalid_argument(std::string(who) + ": " + what); };
  if ((wdf == nullptr) != (bd == nullptr) || (wdf == nullptr) != (yd == nullptr))
    fail("the downsample needs wdf, bd and yd together");
  if (!a.x || !a.wf || !a.bias || !a.y || (S::CI == 64 && !zero) ||
      (((uintptr_t)a.x | (uintptr_t)a.wf | (uintptr_t)wdf | (uintptr_t)a.y | (uintptr_t)yd | (uintptr_t)zero) & 15))
    fail("null / misaligned operand");
  if ((const void*)a.x == (const void*)a.y || (const void*)a.x == yd) fail("in-place not supported");
  if ((long)B * kHI * kWI * S::CI >= (1L << 31)) fail("batch too large");
  void (*kernel)(typename S::Args);
  if constexpr (S::CI == 64)
    kernel = wdf ? conv3x3_s2rows_kernel<S, true, false> : conv3x3_s2rows_kernel<S, false, false>;
  else
    kernel = out8 ? conv3x3_s2rows_kernel<S, false, true> : conv3x3_s2rows_kernel<S, false, false>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(256), S2Derived<S>::kLds, s, a);
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace

bool conv3x3_s2rows_supported(int Hin, int Win, int Cin, int Cout) {
  return Hin == kHI && Win == kWI && Cin == S2Shape64::CI && Cout == kCO;
}

bool conv3x3_s2rows128_supported(int Hin, int Win, int Cin, int Cout) {
  return Hin == kHI && Win == kWI && Cin == S2Shape128::CI && Cout == kCO;
}

void conv3x3_s2rows(const void* x, const void* wf, const float* bias, const void* wdf, const float* bd, void* y,
                    void* yd, const void* zero, int B, bool relu, hipStream_t s) {
  const S2Shape64::Args a{(const bf16*)x,   (const bf16*)wf, (const bf16*)wdf, bias, bd, (bf16*)y, (bf16*)yd,
                          (const bf16*)zero, relu,            kernel_stagger(kStagS2rows)};
  s2rows_launch<S2Shape64>("conv3x3_s2rows", a, wdf, bd, yd, zero, false, B, s);
}

void conv3x3_s2rows128(const void* x, const void* wf, const float* bias, void* y, int B, bool relu,
                       float out_inv_scale, hipStream_t s) {
  const S2Shape128::Args a{(const bf16*)x, (const bf16*)wf, bias, y, relu, out_inv_scale};
  s2rows_launch<S2Shape128>("conv3x3_s2rows128", a, nullptr, nullptr, nullptr, nullptr, out_inv_scale > 0.f, B, s);
}

}  // namespace dmlc
