// Query-batch k x k / stride-1 conv with an optional 3x3/s2 max-pool taken in
// LDS (B <= a few images): AlexNet's features.3 (5x5 / pad 2 on 27x27x64 ->
// 192, + features.5's pool), features.6 / .8 (3x3 / pad 1 on 13x13x192 -> 384,
// 384 -> 256) and features.10 (256 -> 256, + features.12's pool).
//
// Reference equivalent: those Conv2d + ReLU (+ MaxPool2d) modules of
// tch::vision::alexnet, run for ONE image per query by `forward_t`
// (src/services.rs:493). conv_direct.hip keeps an image in one workgroup's LDS:
// at B = 1 one CU works and the rest of the GPU idles for four launches in a
// row. conv_small.hip spreads a conv over the CUs but takes 3x3 only, pixels of
// 2^n chunks and no pool. Here, one launch per conv (+ pool):
//
//  * grid = (Cout/16 channel tiles, pixel tiles, B). A channel tile is one
//    16-row N fragment nf of a 32-channel group g of the fragment-order
//    weights (stream_frag_index, perm32 rows): a lane ends with the 4 output
//    channels 32g + 8fq + 4nf .. +3 of one pixel;
//  * pixel tile without pool: MF x 16 consecutive pixels (MF = 1, 2, 4);
//  * pixel tile with pool: ONE pooled output row r = conv rows 2r, 2r+1, 2r+2,
//    FPR = ceil(W/16) fragments a conv row (13 of 16 / 27 of 32 lanes live),
//    MF = 3 FPR. Seam conv rows are computed by both neighbours; the un-pooled
//    output never exists;
//  * only the input rows the tile reads (all columns, all channels) go to LDS
//    by LDS-DMA. Pixels of more than 128 B are padded to a multiple of 256 B,
//    16-B chunks XOR-swizzled by pixel (xswz, common.h): the 16 pixels of a
//    fragment read 16 distinct bank slots. A tap outside the image (and a dead
//    lane) reads a 256-B zero region at its own bank slot (address select, no
//    VALU on the data): every read is conflict free, border lanes included
//    (tests/test_small_alex_plan_cpu.py);
//  * the 4 waves split K (wave w: K steps w, w+4, ...) and load ALL their
//    weight fragments into registers right after the input DMA (<= 27 x 16 B a
//    lane): every global load of the kernel is in flight at once;
//  * the waves' partial sums meet in LDS as [wave][f][lane]; then + bias,
//    ReLU, bf16. With pool the rounded tile goes to LDS (over the staged rows,
//    which nobody reads any more) and the 3x3/s2 maximum of the bf16 values
//    (>= 0 after the ReLU: an unsigned 16-bit max) is the only thing stored.
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace dmlc {

namespace {

struct SmallKArgs {
  const bf16* x;      // [B, HW, HW, CI]
  const bf16* wf;     // [CO/32][KT][2][64][8] fragment order, K = KS KS CI
  const float* bias;  // [CO]
  bf16* y;            // [B, HW, HW, CO], or pooled [B, PH, PH, CO]
  int CO;
  int relu;
};

template <int KS_, int CI_, int HW_, bool POOL_>
struct SmallKShape {
  static constexpr int KS = KS_, CI = CI_, HW = HW_;
  static constexpr bool POOL = POOL_;
  static constexpr int PAD = KS / 2;
  static constexpr int CPX = CI / 8;                                // 16-B chunks per pixel
  static constexpr int PXC = CPX > 8 ? (CPX + 15) / 16 * 16 : CPX;  // padded chunks per staged pixel
  static constexpr int PXB = PXC * 16;
  static constexpr int KPT = CI / 32;       // K steps per tap
  static constexpr int KT = KS * KS * KPT;  // K steps
  static constexpr int KW = (KT + 3) / 4;   // K steps per wave (at most)
  static constexpr int FPR = (HW + 15) / 16;  // pool: fragments per conv row
  static constexpr int PH = (HW - 3) / 2 + 1;  // pooled rows / columns
  static_assert(CPX == 8 || CPX >= 16, "xswz covers 128-B pixels and pixels of >= 256 B");
  static_assert(KS * KS <= 31, "the tap mask is one int");
  static_assert(KT / 4 + 1 < 64, "vmcnt range");
};

constexpr int kZeroB = 256;  // zero region: one 64-bank window

template <int MF>
constexpr int part_bytes() {
  return 4 * MF * 64 * 16;
}

template <class S, int MF>
__global__ __launch_bounds__(256, 1) void conv_smallk_kernel(SmallKArgs a) {
  constexpr int KS = S::KS, PAD = S::PAD, CI = S::CI, H = S::HW, W = S::HW;
  constexpr int CPX = S::CPX, PXC = S::PXC, PXB = S::PXB, KPT = S::KPT, KT = S::KT, KW = S::KW, FPR = S::FPR;
  constexpr int PART = part_bytes<MF>();
  constexpr int ZOFF = PART;           // 256 zero bytes
  constexpr int ROFF = PART + kZeroB;  // staged input rows (a multiple of 256 B: bank slots as computed)
  static_assert(!S::POOL || MF == 3 * FPR, "a pooled tile is three conv rows");
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  char* lds = (char*)smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int g = blockIdx.x >> 1, nf = blockIdx.x & 1;
  const int b = blockIdx.z;
  // the tile's pixels and the input rows ih_lo .. ih_hi they read
  const int p0 = S::POOL ? 0 : blockIdx.y * (MF * 16);
  const int p1 = S::POOL ? 0 : min(p0 + MF * 16, H * W);
  const int r0 = S::POOL ? 2 * (int)blockIdx.y : p0 / W;        // first conv row
  const int r1 = S::POOL ? r0 + 2 : (p1 - 1) / W;               // last conv row
  const int ih_lo = max(0, r0 - PAD), ih_hi = min(H - 1, r1 + PAD);
  const int total = (ih_hi - ih_lo + 1) * W * PXC;  // staged slots

  // ---- input rows -> LDS: slot s = K PXC + pc holds logical chunk pc ^ xswz(K)
  // of staged pixel K (slots whose logical chunk is past CPX: padding, never read)
  {
    const bf16* src0 = a.x + ((long)(b * H + ih_lo) * W) * CI;
    char* reg = lds + ROFF;
    for (int s0 = wave * 64; s0 < total; s0 += 256) {
      const int s = s0 + lane;
      const int K = s / PXC, pc = s - K * PXC;
      const int lc = pc ^ xswz<CPX>(K);
      if (s < total && lc < CPX) dma16(src0 + (long)K * CI + lc * 8, reg + s0 * 16);
    }
  }
  if (tid < kZeroB / 16) ((uint4*)(lds + ZOFF))[tid] = make_uint4(0, 0, 0, 0);

  // ---- this wave's weight fragments: K steps t = wave + 4 j
  const bf16* wb = a.wf + ((long)g * KT * 2 + nf) * 512 + lane * 8;
  bf16x8 wr[KW];
#pragma unroll
  for (int j = 0; j < KW; ++j) {
    const int t = wave + 4 * j;
    if (KT % 4 == 0 || t < KT) wr[j] = *(const bf16x8*)(wb + (long)t * 1024);
  }

  // ---- per-lane pixel geometry: staged pixel of tap (0, 0) (may lie outside
  // the staged rows) and the taps inside the image (bit kh KS + kw)
  int qb[MF], vm[MF];
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    int oh, ow;
    bool live;
    if constexpr (S::POOL) {
      oh = r0 + f / FPR;
      ow = 16 * (f % FPR) + fr;
      live = ow < W;
    } else {
      const int p = p0 + 16 * f + fr;
      oh = p / W;
      ow = p - oh * W;
      live = p < p1;
    }
    const int ih = oh - PAD, iw = ow - PAD;
    qb[f] = (ih - ih_lo) * W + iw;
    int m = 0;
#pragma unroll
    for (int kh = 0; kh < KS; ++kh)
#pragma unroll
      for (int kw = 0; kw < KS; ++kw)
        m |= ((unsigned)(ih + kh) < (unsigned)H && (unsigned)(iw + kw) < (unsigned)W) << (kh * KS + kw);
    vm[f] = live ? m : 0;
  }

  // the input DMA has landed (only the weight loads, issued after it, may
  // still be in flight: vmcnt retires in order) for every wave (waves with
  // fewer K steps issued fewer loads: wait for the smallest count)
  vm_wait<KT / 4>();
  lds_barrier();

  floatx4 acc[MF];
#pragma unroll
  for (int f = 0; f < MF; ++f) acc[f] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < KW; ++j) {
    const int t = wave + 4 * j;
    if (KT % 4 != 0 && t >= KT) break;
    const int tap = t / KPT;
    const int c = (t - tap * KPT) * 4 + fq;  // logical chunk
    const int kh = tap / KS, kw = tap - kh * KS;
    const int dq = kh * W + kw;
#pragma unroll
    for (int f = 0; f < MF; ++f) {
      const int K = qb[f] + dq;
      const bool ok = (vm[f] >> tap) & 1;
      // a tap outside the image reads zeros at the bank slot its pixel would have
      const int off = K * PXB + ((c ^ xswz<CPX>(K)) << 4);
      const bf16x8 xb = *(const bf16x8*)(lds + (ok ? ROFF + off : ZOFF + (off & (kZeroB - 1))));
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[j], xb, acc[f], 0, 0, 0);
    }
  }

  // ---- the 4 waves' partial sums meet in LDS: [wave][f][lane]
  floatx4* part = (floatx4*)lds;
#pragma unroll
  for (int f = 0; f < MF; ++f) part[(wave * MF + f) * 64 + lane] = acc[f];
  lds_barrier();

  const int ch = 32 * g + 8 * fq + 4 * nf;  // this lane's 4 output channels
  const floatx4 bs = *(const floatx4*)(a.bias + ch);
  auto finish = [&](int f) __attribute__((always_inline)) {
    floatx4 v = bs;
#pragma unroll
    for (int w = 0; w < 4; ++w) v += part[(w * MF + f) * 64 + lane];
    // ReLU on the rounded values as a signed 16-bit max (relu_bf16x8's argument, common.h; -0 becomes +0)
    typedef short short4v __attribute__((ext_vector_type(4)));
    const uint2 u = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
    const short4v z = {0, 0, 0, 0};
    return a.relu ? __builtin_bit_cast(uint2, __builtin_elementwise_max(__builtin_bit_cast(short4v, u), z)) : u;
  };
  if constexpr (!S::POOL) {
    for (int f = wave; f < MF; f += 4) {
      const int p = p0 + 16 * f + fr;
      if (p < p1) *(uint2*)(a.y + ((long)b * (H * W) + p) * a.CO + ch) = finish(f);
    }
  } else {
    // the rounded tile [3 conv rows][16 FPR columns][fq] x 8 B over the staged
    // rows (every wave is past its K loop), then the pooled row
    typedef unsigned short ushort4v __attribute__((ext_vector_type(4)));
    constexpr int PH = S::PH, TW = 16 * FPR;
    static_assert(3 * TW * 32 <= (KS + 2) * W * PXB, "the tile fits the staged rows");
    char* tile = lds + ROFF;
    for (int f = wave; f < MF; f += 4) {
      const int ow = 16 * (f % FPR) + fr;
      if (ow < W) *(uint2*)(tile + (((f / FPR) * TW + ow) * 4 + fq) * 8) = finish(f);
    }
    lds_barrier();
    for (int it = tid; it < PH * 4; it += 256) {
      const int pw = it >> 2, cq = it & 3;
      ushort4v m = ushort4v{0, 0, 0, 0};
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
          m = __builtin_elementwise_max(m, *(const ushort4v*)(tile + ((dy * TW + 2 * pw + dx) * 4 + cq) * 8));
      *(ushort4v*)(a.y + (((long)b * PH + blockIdx.y) * PH + pw) * a.CO + 32 * g + 8 * cq + 4 * nf) = m;
    }
  }
}

// staged input rows of the worst pixel tile
int max_rows(int HW, int pad, int mf) {
  const int P = HW * HW, tp = mf * 16;
  int best = 0;
  for (int p0 = 0; p0 < P; p0 += tp) {
    const int p1 = std::min(p0 + tp, P);
    const int lo = std::max(0, p0 / HW - pad), hi = std::min(HW - 1, (p1 - 1) / HW + pad);
    best = std::max(best, hi - lo + 1);
  }
  return best;
}

template <class S>
size_t lds_bytes(int mf) {
  const int rows = S::POOL ? S::KS + 2 : max_rows(S::HW, S::PAD, mf);
  return (size_t)4 * mf * 64 * 16 + kZeroB + (size_t)rows * S::HW * S::PXB;
}

constexpr size_t kMaxLds = 160 * 1024;

template <class S, int MF>
void launch(const SmallKArgs& a, int B, hipStream_t s) {
  const size_t lds = lds_bytes<S>(MF);
  if (lds > kMaxLds) throw std::invalid_argument("conv_smallk: pixel tile too large for LDS");
  const int tiles = S::POOL ? S::PH : (S::HW * S::HW + MF * 16 - 1) / (MF * 16);
  hipLaunchKernelGGL((conv_smallk_kernel<S, MF>), dim3(a.CO / 16, tiles, B), dim3(256), lds, s, a);
}

template <int KS, int CI, int HW>
void launch_shape(const SmallKArgs& a, int B, int mf, hipStream_t s) {
  using S = SmallKShape<KS, CI, HW, false>;
  switch (mf) {
    case 1: launch<S, 1>(a, B, s); break;
    case 2: launch<S, 2>(a, B, s); break;
    default: launch<S, 4>(a, B, s); break;
  }
}

// 0: 27x27x64 5x5, 1..3: 13x13 x 192 / 384 / 256 3x3; -1: none
int shape_of(int H, int W, int CI, int ks, int pad) {
  if (H == 27 && W == 27 && CI == 64 && ks == 5 && pad == 2) return 0;
  if (H == 13 && W == 13 && ks == 3 && pad == 1) return CI == 192 ? 1 : CI == 384 ? 2 : CI == 256 ? 3 : -1;
  return -1;
}

}  // namespace

bool conv_smallk_supported(int H, int W, int CI, int CO, int ks, int pad, bool pool) {
  const int v = shape_of(H, W, CI, ks, pad);
  if (v < 0 || CO <= 0 || CO % 32 != 0) return false;
  return !pool || v == 0 || v == 3;  // the pooled forms: features.3 and features.10
}

int conv_smallk_pick_mf(int B, int H, int W, int CI, int CO, int ks, int num_cus) {
  (void)CI;
  (void)ks;
  // the widest pixel tile that still gives 1.5 workgroups a CU (fewer, fatter
  // workgroups re-read the weights less often; with fewer than that the narrower
  // tile measured faster: mf = 1 at B = 1, mf = 2 at B = 4, profiles/alex_small.txt)
  for (int mf : {4, 2})
    if (2 * (long)(CO / 16) * ((H * W + mf * 16 - 1) / (mf * 16)) * B >= 3 * num_cus) return mf;
  return 1;
}

void conv_smallk(const void* x, const void* wf, const float* bias, void* y, int B, int H, int W, int CI, int CO, int ks,
                 int pad, bool relu, bool pool, int mf, hipStream_t s) {
  if (B <= 0) return;
  if (!conv_smallk_supported(H, W, CI, CO, ks, pad, pool)) throw std::invalid_argument("conv_smallk: unsupported shape");
  if (pool && !relu) throw std::invalid_argument("conv_smallk: the fused max-pool needs ReLU");
  if (!x || !wf || !bias || !y) throw std::invalid_argument("conv_smallk: null operand");
  if (((uintptr_t)x | (uintptr_t)wf | (uintptr_t)y) & 15)
    throw std::invalid_argument("conv_smallk: operands must be 16-B aligned");
  if ((uintptr_t)bias & 15) throw std::invalid_argument("conv_smallk: bias must be 16-B aligned");
  if (!pool && mf != 1 && mf != 2 && mf != 4) throw std::invalid_argument("conv_smallk: mf must be 1, 2 or 4");
  const int Ho = pool ? (H - 3) / 2 + 1 : H;
  // a workgroup stages its rows while others already store theirs
  if (ranges_overlap(x, (size_t)B * H * W * CI * 2, y, (size_t)B * Ho * Ho * CO * 2))
    throw std::invalid_argument("conv_smallk: in-place not supported");
  if ((long)B * H * W * CI >= (1L << 31) || (long)B * Ho * Ho * CO >= (1L << 31))
    throw std::invalid_argument("conv_smallk: tensor too large for 32-bit offsets");
  if (B > 65535) throw std::invalid_argument("conv_smallk: batch too large");
  const SmallKArgs a{(const bf16*)x, (const bf16*)wf, bias, (bf16*)y, CO, relu ? 1 : 0};
  switch (shape_of(H, W, CI, ks, pad)) {
    case 0:
      if (pool) launch<SmallKShape<5, 64, 27, true>, 6>(a, B, s);
      else launch_shape<5, 64, 27>(a, B, mf, s);
      break;
    case 1: launch_shape<3, 192, 13>(a, B, mf, s); break;
    case 2: launch_shape<3, 384, 13>(a, B, mf, s); break;
    default:
      if (pool) launch<SmallKShape<3, 256, 13, true>, 3>(a, B, s);
      else launch_shape<3, 256, 13>(a, B, mf, s);
      break;
  }
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
