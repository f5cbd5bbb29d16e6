// Nearest-neighbour search over embeddings: queries x an HBM-resident bf16
// gallery on the MFMA, keeping only each query's k best rows. The [B, N]
// score matrix never exists.
//
// Reference counterpart: none (the reference answers with a class name only,
// src/services.rs:493-497). What torch users write instead is q @ g.T into a
// [B, N] fp32 matrix in HBM, then torch.topk over it.
//
// score(b, n) = (sum_d bf16(q[b][d]) g[n][d]) q_scale[b] g_scale[n]: exact
// products, fp32 accumulation on v_mfma_f32_16x16x32_bf16 over the whole of D
// by one wave in one K order (no split-K), then the two fp32 multiplies in
// that order (a null scale multiplies by 1, which is exact). So a score's
// bits do not depend on B, N, the row's place in its tile or the slice count.
// Row b of the answer: the k largest scores in descending order, equal scores
// by ascending n (softmax_topk's tie rule at every rank). Inputs are assumed
// finite: -inf marks an empty slot, and a NaN never wins a comparison.
//
// sim_topk_kernel. A workgroup owns one block of <= 256 queries and one
// slice of the gallery: contiguous whole tiles of 128 rows, about one
// workgroup per CU. fc_gemm.hip's loop with the operands' roles swapped:
//
//  * a stage is one K block (64) of the tile's 128 gallery rows (16 KB) and of
//    the 256 queries (32 KB, L2-resident, re-read per tile), brought to a
//    2-slot LDS ring by LDS-DMA, 16-B chunks XOR-swizzled by row through the
//    source addresses; the stages run on across tile boundaries, so the next
//    tile's first block loads under the current tile's last block and its
//    selection. (Two slots, one stage in flight: three would leave no LDS for
//    the lists below.) Rows past N or B and the missing half of a last K
//    block of 32 repeat a valid address: nothing is read out of bounds, what
//    lands is never used;
//  * wave w owns queries 32 w .. 32 w + 31 against all 128 gallery rows: the
//    gallery is the MFMA's A operand, so lane (fr, fq) holds, per query
//    fragment, the scores of query fr against gallery rows 4 fq + r of all 8
//    row fragments: 64 accumulator registers, 16 MFMAs per 10 fragment reads.
//    A query belongs to one wave only, so nothing below is shared between
//    waves; waves whose queries all lie past B only help with the DMA;
//  * selection: each query's sorted k-entry (score, n) list lives in LDS and
//    its k-th score (the threshold) in a register of the query's 4 lanes. After
//    a tile a lane compares its 64 scores with its thresholds; only when the
//    wave's ballot finds a beat does it take the slow path, where the 4 lanes
//    of a query take turns to insert their candidates (the exact comparison,
//    ties included, is made again against the list). Tiles arrive in
//    ascending n, so "strictly above the threshold at the tile's start" loses
//    no tie. Past the first tiles almost nothing beats the threshold;
//  * g_scale's 128 values of a tile ride along with the tile's first stage
//    (two 4-B DMAs) into a 2-deep LDS buffer.
//
// One slice writes the answer itself. Otherwise every slice writes its k
// candidates per query to the workspace and sim_merge_kernel, one wave per
// query, merges the slices' sorted lists: a lane holds the heads of its
// slices, the (value, index) arg-max butterfly picks the next rank, the
// winner's lane advances that head. The comparisons are the same total order
// on (score, n), so the answer is bit-identical for every slice count.
//
// The row filter (FILTER): g_label[n] < 0 marks a removed row, and a query
// with want >= 0 accepts only rows labelled want. A tile's 128 labels ride
// with its first stage as the scales do; after the scaling step a score whose
// row fails its query's filter becomes -inf, exactly what a row past N is, so
// the threshold, ballot and insertion logic never see it (-inf > thr is false
// even for thr = -inf). A query with fewer than k candidates keeps empty
// slots (-inf, INT_MAX) at the end of its list; whatever writes the answer
// (this kernel at one slice, else the merge) turns their INT_MAX into -1.
// The FILTER = false instantiations are the unfiltered kernels unchanged.
//
// The e4m3 gallery (FP8): one byte per element. A row is stored as OCP e4m3fn
// codes c = e4m3_rne(v 2^e), e the largest integer with max|v| 2^e <= 448
// (clamped to +-126; 0 for a zero row), and one fp32 scale: 2^-e (dot) or
// 1 / max(sqrt(sum c^2), 1e-12) (cosine: the power of two cancels). Queries
// are quantised by the same rule (gallery_pack8, into the workspace), and
// score(b, n) = ((sum_d cq[b][d] cg[n][d]) q_scale[b]) g_scale[n] on
// v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales, at twice the bf16
// rate per clock and half the bytes. The stage geometry is byte-identical: a
// 128-B LDS row holds a K block of 128 codes, and a lane's operand is chunks
// fq and fq + 4 of its row (the pair that keeps the 16 lanes of a ds_read_b128
// group on distinct banks under the row swizzle: chunks 2 fq, 2 fq + 1 would
// pair lanes whose chunk numbers differ in bit 1 only). The MFMA takes lane
// (fr, fq)'s 32 bytes as K = 32 fq .. 32 fq + 31 of its row; both operands
// read the same chunks, so which K a byte stands for cancels in the sum.
// Selection, filter, slices and the merge are the bf16 kernel's code.
//
// gallery_pack8: one wave per row; pass 1 finds max|v| across the wave, pass 2
// scales (exact), converts with v_cvt_pk_fp8_f32 and sums the squares of the
// decoded codes as gallery_pack does.
//
// gallery_pack: fp32 rows -> bf16 (nearest even), optionally with
// 1 / max(sqrt(sum v^2), 1e-12) of the rounded values v (fp32 squares summed
// per lane and across the wave; IEEE root and divide): embed.hip's
// normalisation rule on what the MFMA will read. One wave per row.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <climits>
#include <type_traits>

namespace dmlc {

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));

constexpr int kBQ = 256;  // queries per workgroup
constexpr int kBG = 128;  // gallery rows per tile
constexpr int kKB = 64;   // K block per stage (bf16)
constexpr int kKB8 = 128;  // K block per stage (e4m3): the same 128 bytes a row
constexpr int kGB = kBG * kKB * 2;  // 16 KB gallery stage
constexpr int kQB = kBQ * kKB * 2;  // 32 KB query stage
constexpr int kStage = kGB + kQB;
constexpr int kSlots = 2;
constexpr int kListS = kSlots * kStage;              // float [kBQ][kMaxTopK]
constexpr int kListI = kListS + kBQ * kMaxTopK * 4;  // int   [kBQ][kMaxTopK]
constexpr int kGScale = kListI + kBQ * kMaxTopK * 4;  // float [2][kBG]
constexpr int kGLabel = kGScale + 2 * kBG * 4;  // int   [2][kBG] (FILTER)
constexpr int kLdsPlain = kGLabel;               // what the unfiltered kernel is launched with
constexpr int kLds = kGLabel + 2 * kBG * 4;
constexpr int kMaxSlices = 512;  // 8 heads a lane in the merge
constexpr int kMaxD = 4096;
static_assert(kLds <= 160 * 1024, "LDS per CU");
static_assert(kMaxTopK == 16, "list rows of 16 entries");

// 16-B chunk c (0..7) of a 128-B LDS row r
__device__ __forceinline__ int st_off(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }

// (s, n) sorts before (ps, pn): the larger score, the lower row among equals
__device__ __forceinline__ bool sorts_before(float s, int n, float ps, int pn) {
  return s > ps || (s == ps && n < pn);
}

// Insert (s, n) into a sorted k-entry list unless it sorts after its last entry.
__device__ __forceinline__ void list_insert(float* ls, int* li, int k, float s, int n) {
  if (!sorts_before(s, n, ls[k - 1], li[k - 1])) return;
  int pos = k - 1;
  while (pos > 0) {
    const float ps = ls[pos - 1];
    const int pn = li[pos - 1];
    if (!sorts_before(s, n, ps, pn)) break;
    ls[pos] = ps;
    li[pos] = pn;
    --pos;
  }
  ls[pos] = s;
  li[pos] = n;
}

// q: bf16 [Bq, D], this block's queries; g: bf16 [N, D]. Slice blockIdx.x of
// gridDim.x takes tiles [t0, t1). out_s / out_i: [Bq][gridDim.x][k].
// FILTER: g_label [N] (never null), q_want [Bq] or null.
// FP8: q and g hold e4m3 codes (D % 128 == 0), both scales are given.
template <bool FP8>
using sim_elem = typename std::conditional<FP8, uint8_t, bf16>::type;

template <bool SCALED, bool FILTER, bool FP8 = false>
__global__ __launch_bounds__(512, 1) void sim_topk_kernel(const sim_elem<FP8>* __restrict__ q,
                                                          const float* __restrict__ q_scale,
                                                          const sim_elem<FP8>* __restrict__ g,
                                                          const float* __restrict__ g_scale, int Bq, long N, int D,
                                                          int k, float* __restrict__ out_s,
                                                          int32_t* __restrict__ out_i,
                                                          const int32_t* __restrict__ g_label,
                                                          const int32_t* __restrict__ q_want) {
  static_assert(!FP8 || SCALED, "e4m3 codes always come with their scales");
  constexpr int KB = FP8 ? kKB8 : kKB;  // K elements per stage
  constexpr int CE = FP8 ? 16 : 8;      // elements per 16-B chunk
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];
  char* lds = (char*)smem;
  float* ls = (float*)(lds + kListS);
  int* li = (int*)(lds + kListI);
  float* gsl = (float*)(lds + kGScale);
  int* gll = (int*)(lds + kGLabel);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int slices = gridDim.x, slice = blockIdx.x;
  const long tiles = (N + kBG - 1) / kBG;
  const long base_t = tiles / slices, rem = tiles % slices;
  const long t0 = slice * base_t + (slice < rem ? slice : rem);
  const int nt = (int)(base_t + (slice < rem ? 1 : 0));
  const int nk = (D + KB - 1) / KB;
  const bool active = 32 * wave < Bq;  // (wave-uniform)

  // this wave's lists start empty; without g_scale the scale buffer holds ones
  for (int e = lane; e < 32 * kMaxTopK; e += 64) {
    ls[32 * wave * kMaxTopK + e] = -INFINITY;
    li[32 * wave * kMaxTopK + e] = INT_MAX;
  }
  if (SCALED && !g_scale && tid < 2 * kBG) gsl[tid] = 1.f;
  float thr[2], qs[2];
  int want[2];  // (FILTER) >= 0: the only label the query accepts
#pragma unroll
  for (int qf = 0; qf < 2; ++qf) {
    const int b = 32 * wave + 16 * qf + fr;
    thr[qf] = b < Bq ? -INFINITY : INFINITY;  // a query past B never has a candidate
    qs[qf] = SCALED && q_scale && b < Bq ? q_scale[b] : 1.f;
    want[qf] = FILTER && q_want && b < Bq ? q_want[b] : -1;
  }
  lgkm_wait();

  // Staging (fc_gemm.hip's): LDS position p = 64 i + l of a region holds row
  // p >> 3, physical chunk p & 7 = logical chunk (p & 7) ^ (row & 7). The
  // gallery region is 16 instructions (2 a wave), the query region 32 (4 a
  // wave; those whose 8 rows all lie past Bq are skipped). Every wait is
  // vmcnt(0), so the waves need not issue the same number.
  auto dma_stage = [&](long tile, int kb, int slot) __attribute__((always_inline)) {
    char* base = lds + slot * kStage;
    const int k0 = kb * KB;
    const long n0 = tile * kBG;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int p = (2 * wave + j) * 64 + lane, r = p >> 3;
      int kc = k0 + CE * ((p & 7) ^ (r & 7));
      if (!FP8 && kc >= D) kc -= 32;  // (the absent half of a last block of 32)
      const long row = n0 + r < N ? n0 + r : N - 1;
      dma16(g + row * D + kc, base + (2 * wave + j) * 1024);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = 4 * wave + j;
      if (8 * i < Bq) {
        const int p = i * 64 + lane, r = p >> 3;
        int kc = k0 + CE * ((p & 7) ^ (r & 7));
        if (!FP8 && kc >= D) kc -= 32;
        const int row = r < Bq ? r : Bq - 1;
        dma16(q + (long)row * D + kc, base + kGB + i * 1024);
      }
    }
    if (SCALED && g_scale && kb == 0 && wave < 2) {
      const long n = n0 + 64 * wave + lane;
      dma4(g_scale + (n < N ? n : N - 1), gsl + (tile & 1) * kBG + 64 * wave);
    }
    if (FILTER && kb == 0 && wave < 2) {
      const long n = n0 + 64 * wave + lane;
      dma4(g_label + (n < N ? n : N - 1), gll + (tile & 1) * kBG + 64 * wave);
    }
  };

  floatx4 acc[8][2];
#pragma unroll
  for (int gf = 0; gf < 8; ++gf)
#pragma unroll
    for (int qf = 0; qf < 2; ++qf) acc[gf][qf] = floatx4{0.f, 0.f, 0.f, 0.f};

  dma_stage(t0, 0, 0);
  int kb = 0, slot = 0;
  for (int t = 0; t < nt;) {
    // this wave's DMA of this stage has landed, after the barrier everyone's
    // has, and every wave is done with the previous stage, whose slot (and,
    // at a tile's first block, whose tile's scale and label buffers) the next DMA reuses
    vm_wait<0>();
    __builtin_amdgcn_s_barrier();
    if (kb + 1 < nk) dma_stage(t0 + t, kb + 1, slot ^ 1);
    else if (t + 1 < nt) dma_stage(t0 + t + 1, 0, slot ^ 1);
    if (active) {
      const char* base = lds + slot * kStage;
      if constexpr (FP8) {
        // the whole K block in one MFMA per fragment pair: chunks fq and fq + 4 of each row
        auto frag = [&](const char* region, int row) __attribute__((always_inline)) {
          const uint4 lo = *(const uint4*)(region + st_off(row, fq));
          const uint4 hi = *(const uint4*)(region + st_off(row, fq + 4));
          return v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        };
        v8i gfr[8], qfr[2];
#pragma unroll
        for (int gf = 0; gf < 8; ++gf) gfr[gf] = frag(base, 16 * gf + fr);
#pragma unroll
        for (int qf = 0; qf < 2; ++qf) qfr[qf] = frag(base + kGB, 32 * wave + 16 * qf + fr);
#pragma unroll
        for (int gf = 0; gf < 8; ++gf)
#pragma unroll
          for (int qf = 0; qf < 2; ++qf)
            acc[gf][qf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(gfr[gf], qfr[qf], acc[gf][qf], 0, 0, 0, 127,
                                                                           0, 127);
      } else {
#pragma unroll
        for (int kk = 0; kk < kKB / 32; ++kk) {
          if (kb * kKB + 32 * kk < D) {  // (uniform)
            bf16x8 gfr[8], qfr[2];
#pragma unroll
            for (int gf = 0; gf < 8; ++gf) gfr[gf] = *(const bf16x8*)(base + st_off(16 * gf + fr, 4 * kk + fq));
#pragma unroll
            for (int qf = 0; qf < 2; ++qf)
              qfr[qf] = *(const bf16x8*)(base + kGB + st_off(32 * wave + 16 * qf + fr, 4 * kk + fq));
#pragma unroll
            for (int gf = 0; gf < 8; ++gf)
#pragma unroll
              for (int qf = 0; qf < 2; ++qf)
                acc[gf][qf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gfr[gf], qfr[qf], acc[gf][qf], 0, 0, 0);
          }
        }
      }
    }
    lgkm_wait();  // (this wave's reads of the slot are done)
    slot ^= 1;
    if (++kb < nk) continue;
    kb = 0;
    // ---- the tile is complete: acc[gf][qf][r] = query 32 wave + 16 qf + fr . gallery row n0 + 16 gf + 4 fq + r
    const long n0 = (t0 + t) * kBG;
    if (active) {
      if constexpr (SCALED) {
        const float* gs = gsl + ((t0 + t) & 1) * kBG;
#pragma unroll
        for (int gf = 0; gf < 8; ++gf) {
          const floatx4 sc = *(const floatx4*)(gs + 16 * gf + 4 * fq);
#pragma unroll
          for (int qf = 0; qf < 2; ++qf)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[gf][qf][r] = (acc[gf][qf][r] * qs[qf]) * sc[r];
        }
      }
      if constexpr (FILTER) {  // a row that fails the query's filter is no candidate
        const int* gl = gll + ((t0 + t) & 1) * kBG;
#pragma unroll
        for (int gf = 0; gf < 8; ++gf) {
          const intx4 lb = *(const intx4*)(gl + 16 * gf + 4 * fq);
#pragma unroll
          for (int qf = 0; qf < 2; ++qf)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (lb[r] < 0 || (want[qf] >= 0 && lb[r] != want[qf])) acc[gf][qf][r] = -INFINITY;
        }
      }
      if (n0 + kBG > N) {  // (uniform) a partial tile: rows past N are no candidates
#pragma unroll
        for (int gf = 0; gf < 8; ++gf)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n0 + 16 * gf + 4 * fq + r >= N) acc[gf][0][r] = acc[gf][1][r] = -INFINITY;
      }
      // bit 32 qf + 4 gf + r: that score beats its query's threshold
      uint64_t mask = 0;
#pragma unroll
      for (int qf = 0; qf < 2; ++qf)
#pragma unroll
        for (int gf = 0; gf < 8; ++gf)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (acc[gf][qf][r] > thr[qf]) mask |= 1ull << (32 * qf + 4 * gf + r);
      if (__ballot(mask != 0)) {
        // the 4 lanes of a query (fq = 0..3) take turns; LDS operations of one
        // wave complete in order, so a turn sees the lists the last one left
        for (int turn = 0; turn < 4; ++turn) {
          if (fq == turn) {
            while (mask) {
              const int j = __builtin_ctzll(mask);
              mask &= mask - 1;
              float s = 0.f;
#pragma unroll
              for (int qf = 0; qf < 2; ++qf)
#pragma unroll
                for (int gf = 0; gf < 8; ++gf)
#pragma unroll
                  for (int r = 0; r < 4; ++r) s = j == 32 * qf + 4 * gf + r ? acc[gf][qf][r] : s;
              const int ql = 32 * wave + 16 * (j >> 5) + fr;
              const int n = (int)(n0 + 16 * ((j >> 2) & 7) + 4 * fq + (j & 3));
              list_insert(ls + ql * kMaxTopK, li + ql * kMaxTopK, k, s, n);
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int qf = 0; qf < 2; ++qf) {
          const int b = 32 * wave + 16 * qf + fr;
          if (b < Bq) thr[qf] = ls[b * kMaxTopK + k - 1];
        }
      }
#pragma unroll
      for (int gf = 0; gf < 8; ++gf)
#pragma unroll
        for (int qf = 0; qf < 2; ++qf) acc[gf][qf] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    ++t;
  }

  // this wave's lists -> [Bq][slices][k]
  if (active) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int e = lane; e < 32 * k; e += 64) {
      const int b = 32 * wave + e / k, j = e % k;
      if (b < Bq) {
        const long o = ((long)b * slices + slice) * k + j;
        out_s[o] = ls[b * kMaxTopK + j];
        const int n = li[b * kMaxTopK + j];
        out_i[o] = FILTER && slices == 1 && n == INT_MAX ? -1 : n;  // (an empty rank of the answer itself)
      }
    }
  }
}

// (v, i) across the wave: the largest value, the lowest index among equals
__device__ __forceinline__ void wave_argmax(float& best, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
}

// cs / ci: [B][slices][k], every slice's list sorted; one wave per query.
// FILTER: lists may end in empty slots (-inf, INT_MAX), written as idx -1.
template <bool FILTER>
__global__ __launch_bounds__(256) void sim_merge_kernel(const float* __restrict__ cs, const int32_t* __restrict__ ci,
                                                        int B, int slices, int k, int32_t* __restrict__ idx,
                                                        float* __restrict__ score) {
  constexpr int H = kMaxSlices / 64;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* s = cs + (long)b * slices * k;
  const int32_t* n = ci + (long)b * slices * k;
  float hv[H];
  int hi[H], hp[H];  // lane's slice lane + 64 j: its head's score, row and position
#pragma unroll
  for (int j = 0; j < H; ++j) {
    const int sl = lane + 64 * j;
    hp[j] = 0;
    hv[j] = sl < slices ? s[(long)sl * k] : -INFINITY;
    hi[j] = sl < slices ? n[(long)sl * k] : INT_MAX;
  }
  int my_i = 0;
  float my_v = 0.f;  // lane r keeps rank r
  for (int r = 0; r < k; ++r) {
    float best = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int j = 0; j < H; ++j)
      if (hv[j] > best || (hv[j] == best && hi[j] < bi)) {
        best = hv[j];
        bi = hi[j];
      }
    wave_argmax(best, bi);
    if (lane == r) {
      my_i = bi;
      my_v = best;
    }
    // rows are distinct across slices, so one head at most is the winner,
    // unless (FILTER) the winner is the empty slot (-inf, INT_MAX): then every
    // head is empty, all of them advance, and as the lists are sorted what
    // follows an empty slot is empty too, so nothing is skipped
#pragma unroll
    for (int j = 0; j < H; ++j) {
      const int sl = lane + 64 * j;
      if (sl < slices && hi[j] == bi && hv[j] == best) {
        ++hp[j];
        hv[j] = hp[j] < k ? s[(long)sl * k + hp[j]] : -INFINITY;
        hi[j] = hp[j] < k ? n[(long)sl * k + hp[j]] : INT_MAX;
      }
    }
  }
  if (lane < k) {
    idx[(long)b * k + lane] = FILTER && my_i == INT_MAX ? -1 : my_i;
    score[(long)b * k + lane] = my_v;
  }
}

// One wave per row, 4 rows a workgroup; a lane owns 8-element groups lane, lane + 64, ...
template <bool IN_BF16>
__global__ __launch_bounds__(256) void gallery_pack_kernel(const void* __restrict__ rows, bf16* __restrict__ g,
                                                           float* __restrict__ inv_norm, int M, int D) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  float ss = 0.f;
  for (int c = lane * 8; c < D; c += 512) {
    float v[8];
    if constexpr (IN_BF16) {
      unpack8(*(const uint4*)((const bf16*)rows + (long)m * D + c), v);
    } else {
      const float4* src = (const float4*)((const float*)rows + (long)m * D + c);
      const float4 lo = src[0], hi = src[1];
      const float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      const uint4 p = pack8(f);
      *(uint4*)(g + (long)m * D + c) = p;
      unpack8(p, v);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
  }
  if (inv_norm) {  // (uniform)
    ss = wave_sum(ss);
    if (lane == 0) inv_norm[m] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
  }
}

// 8 consecutive values of row m as fp32 (a bf16 input widens exactly)
template <bool IN_BF16>
__device__ __forceinline__ void load8(const void* rows, long at, float* v) {
  if constexpr (IN_BF16) {
    unpack8(*(const uint4*)((const bf16*)rows + at), v);
  } else {
    const float4* src = (const float4*)((const float*)rows + at);
    const float4 lo = src[0], hi = src[1];
    v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w;
    v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
  }
}

// The e4m3 quantiser: one wave per row, 4 rows a workgroup, a lane owns
// 8-element groups lane, lane + 64, ... (16- or 32-B loads, 8-B stores).
// scale[m] = 2^-e (dot) or the inverse norm of the codes (cosine).
template <bool IN_BF16>
__global__ __launch_bounds__(256) void gallery_pack8_kernel(const void* __restrict__ rows, uint8_t* __restrict__ codes,
                                                            float* __restrict__ scale, int M, int D, bool cosine) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  float amax = 0.f;
  for (int c = lane * 8; c < D; c += 512) {
    float v[8];
    load8<IN_BF16>(rows, (long)m * D + c, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
  }
  amax = wave_max(amax);
  // amax = m 2^x, 1 <= m < 2: e = 8 - x, one less if m > 1.75 (448 = 1.75 2^8); a subnormal amax clamps at 126
  const uint32_t ab = __float_as_uint(amax);
  const int x = (int)(ab >> 23) - 127;
  int e = (ab & 0x7fffffu) <= 0x600000u ? 8 - x : 7 - x;
  e = e > 126 ? 126 : e;  // (e >= -120 for any finite amax)
  if (ab == 0) e = 0;
  const float up = __uint_as_float((uint32_t)(127 + e) << 23);  // 2^e
  float ss = 0.f;
  for (int c = lane * 8; c < D; c += 512) {
    float v[8];
    load8<IN_BF16>(rows, (long)m * D + c, v);
    u32x2 p;
    p.x = e4m3x4_from_f32(v[0] * up, v[1] * up, v[2] * up, v[3] * up);
    p.y = e4m3x4_from_f32(v[4] * up, v[5] * up, v[6] * up, v[7] * up);
    *(u32x2*)(codes + (long)m * D + c) = p;
    e4m3x4_to_f32(p.x, v);
    e4m3x4_to_f32(p.y, v + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
  }
  if (cosine) {  // (uniform)
    ss = wave_sum(ss);
    if (lane == 0) scale[m] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
  } else if (lane == 0) {
    scale[m] = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e
  }
}

// labels[ids[i]] = -1: a removed row (equal ids write the same value)
__global__ __launch_bounds__(256) void gallery_unlabel_kernel(int32_t* __restrict__ labels,
                                                              const int32_t* __restrict__ ids, int M, long N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const int n = ids[i];
  if (n >= 0 && n < N) labels[n] = -1;
}

long sim_tiles(long N) { return (N + kBG - 1) / kBG; }

size_t align256(size_t n) { return (n + 255) / 256 * 256; }

// The search launches on prepared operands: one per block of 256 queries, then the merge.
template <bool FP8>
void launch_search(const sim_elem<FP8>* qb, const float* q_scale, const sim_elem<FP8>* g, const float* g_scale, int B,
                   long N, int D, int k, int32_t* idx, float* score, float* cs, int32_t* ci, int slices,
                   const int32_t* g_label, const int32_t* q_want, hipStream_t s) {
  const bool scaled = q_scale || g_scale;
  for (int b0 = 0; b0 < B; b0 += kBQ) {  // blocks of 256 queries
    const int Bq = std::min(kBQ, B - b0);
    // one slice: the lists are the answer ([Bq][1][k] = [Bq][k])
    float* os = slices == 1 ? score + (long)b0 * k : cs + (long)b0 * slices * k;
    int32_t* oi = slices == 1 ? idx + (long)b0 * k : ci + (long)b0 * slices * k;
    const float* qsc = q_scale ? q_scale + b0 : nullptr;
    const int32_t* qw = q_want ? q_want + b0 : nullptr;
    auto launch = [&](auto kernel, int lds_bytes) {
      hipLaunchKernelGGL(kernel, dim3(slices), dim3(512), (size_t)lds_bytes, s, qb + (long)b0 * D, qsc, g, g_scale, Bq,
                         N, D, k, os, oi, g_label, qw);
    };
    if constexpr (FP8) {
      if (g_label) launch(sim_topk_kernel<true, true, true>, kLds);
      else launch(sim_topk_kernel<true, false, true>, kLdsPlain);
    } else if (g_label) {
      if (scaled) launch(sim_topk_kernel<true, true>, kLds);
      else launch(sim_topk_kernel<false, true>, kLds);
    } else {
      if (scaled) launch(sim_topk_kernel<true, false>, kLdsPlain);
      else launch(sim_topk_kernel<false, false>, kLdsPlain);
    }
    DMLC_HIP_CHECK(hipGetLastError());
  }
  if (slices > 1) {
    if (g_label)
      hipLaunchKernelGGL(sim_merge_kernel<true>, dim3((B + 3) / 4), dim3(256), 0, s, (const float*)cs,
                         (const int32_t*)ci, B, slices, k, idx, score);
    else
      hipLaunchKernelGGL(sim_merge_kernel<false>, dim3((B + 3) / 4), dim3(256), 0, s, (const float*)cs,
                         (const int32_t*)ci, B, slices, k, idx, score);
    DMLC_HIP_CHECK(hipGetLastError());
  }
}

}  // namespace

bool sim_topk_supported(int D) { return D >= 32 && D <= kMaxD && D % 32 == 0; }

int sim_topk_max_slices(long N) { return N < 1 ? 0 : (int)std::min<long>(sim_tiles(N), kMaxSlices); }

int sim_topk_slices(int B, long N, int num_cus) {
  (void)B;  // every block of 256 queries is its own launch of this many workgroups
  if (N < 1) return 0;
  return std::max(1, std::min(sim_topk_max_slices(N), num_cus));
}

void sim_topk_slice_rows(long N, int slices, int slice, long* first, long* end) {
  if (N < 1 || slices < 1 || slices > sim_topk_max_slices(N) || slice < 0 || slice >= slices)
    throw std::invalid_argument("sim_topk_slice_rows: bad slice");
  const long tiles = sim_tiles(N), base = tiles / slices, rem = tiles % slices;
  const long t0 = slice * base + std::min<long>(slice, rem), t1 = t0 + base + (slice < rem ? 1 : 0);
  *first = t0 * kBG;
  *end = std::min(N, t1 * kBG);
}

size_t sim_topk_ws_bytes(int B, int k, int slices) {
  if (B < 0 || k < 0 || slices < 0) throw std::invalid_argument("sim_topk_ws_bytes: negative argument");
  // the candidates' scores and rows [B][slices][k], then the queries as bf16 at the widest D
  return 2 * align256((size_t)slices * B * k * 4) + (size_t)B * kMaxD * 2;
}

bool sim_topk8_supported(int D) { return D >= kKB8 && D <= kMaxD && D % kKB8 == 0; }

size_t sim_topk8_ws_bytes(int B, int k, int slices) {
  if (B < 0 || k < 0 || slices < 0) throw std::invalid_argument("sim_topk8_ws_bytes: negative argument");
  // the candidates as above, then the queries' codes at the widest D and their scales
  return 2 * align256((size_t)slices * B * k * 4) + (size_t)B * (kMaxD + 4);
}

void gallery_pack(const float* rows, void* g, float* inv_norm, int M, int D, hipStream_t s) {
  if (D < 8 || D % 8 || D > 8192) throw std::invalid_argument("gallery_pack: needs D % 8 == 0, 8 <= D <= 8192");
  if (M < 0) throw std::invalid_argument("gallery_pack: M < 0");
  if (M == 0) return;
  if (!rows || !g || (uintptr_t)rows % 16 || (uintptr_t)g % 16)
    throw std::invalid_argument("gallery_pack: null / misaligned rows or g (16 B)");
  hipLaunchKernelGGL(gallery_pack_kernel<false>, dim3((M + 3) / 4), dim3(256), 0, s, (const void*)rows, (bf16*)g,
                     inv_norm, M, D);
  DMLC_HIP_CHECK(hipGetLastError());
}

void gallery_unlabel(int32_t* labels, const int32_t* ids, int M, long N, hipStream_t s) {
  if (M < 0 || N < 0) throw std::invalid_argument("gallery_unlabel: negative size");
  if (M == 0) return;
  if (!labels || !ids) throw std::invalid_argument("gallery_unlabel: null labels or ids");
  hipLaunchKernelGGL(gallery_unlabel_kernel, dim3((M + 255) / 256), dim3(256), 0, s, labels, ids, M, N);
  DMLC_HIP_CHECK(hipGetLastError());
}

void gallery_inv_norms(const void* rows_bf16, float* inv_norm, int M, int D, hipStream_t s) {
  if (D < 8 || D % 8 || D > 8192) throw std::invalid_argument("gallery_inv_norms: needs D % 8 == 0, 8 <= D <= 8192");
  if (M < 0) throw std::invalid_argument("gallery_inv_norms: M < 0");
  if (M == 0) return;
  if (!rows_bf16 || !inv_norm || (uintptr_t)rows_bf16 % 16)
    throw std::invalid_argument("gallery_inv_norms: null / misaligned rows (16 B) or null inv_norm");
  hipLaunchKernelGGL(gallery_pack_kernel<true>, dim3((M + 3) / 4), dim3(256), 0, s, rows_bf16, (bf16*)nullptr,
                     inv_norm, M, D);
  DMLC_HIP_CHECK(hipGetLastError());
}

void sim_topk(const void* q, TensorDType qdt, const float* q_scale, const void* g, const float* g_scale, int B, long N,
              int D, int k, int32_t* idx, float* score, void* ws, size_t ws_bytes, int num_cus, hipStream_t s,
              int slices_override, const int32_t* g_label, const int32_t* q_want) {
  if (!sim_topk_supported(D)) throw std::invalid_argument("sim_topk: needs D % 32 == 0, 32 <= D <= 4096");
  if (qdt != TensorDType::F32 && qdt != TensorDType::BF16) throw std::invalid_argument("sim_topk: queries are fp32 or bf16");
  if (B < 0) throw std::invalid_argument("sim_topk: B < 0");
  if (N < 1 || N > INT_MAX) throw std::invalid_argument("sim_topk: N outside 1..2^31 - 1");
  if (k < 1 || k > N || k > kMaxTopK) throw std::invalid_argument("sim_topk: k must be in 1..min(N, kMaxTopK)");
  if (q_want && !g_label) throw std::invalid_argument("sim_topk: q_want needs g_label");
  if (B == 0) return;
  if (!q || !g || !idx || !score || !ws || (((uintptr_t)q | (uintptr_t)g | (uintptr_t)ws) & 15))
    throw std::invalid_argument("sim_topk: null / misaligned operand (q, g and ws need 16 B)");
  const int slices = slices_override ? slices_override : sim_topk_slices(B, N, num_cus);
  if (slices < 1 || slices > sim_topk_max_slices(N))
    throw std::invalid_argument("sim_topk: slices outside 1..min(tiles, 512)");
  if (ws_bytes < sim_topk_ws_bytes(B, k, slices)) throw std::invalid_argument("sim_topk: workspace too small");
  const size_t cand = align256((size_t)slices * B * k * 4);
  float* cs = (float*)ws;
  int32_t* ci = (int32_t*)((char*)ws + cand);
  const bf16* qb = (const bf16*)q;
  if (qdt == TensorDType::F32) {
    void* packed = (char*)ws + 2 * cand;
    gallery_pack((const float*)q, packed, nullptr, B, D, s);
    qb = (const bf16*)packed;
  }
  launch_search<false>(qb, q_scale, (const bf16*)g, g_scale, B, N, D, k, idx, score, cs, ci, slices, g_label, q_want, s);
}

void gallery_pack8(const void* rows, TensorDType dt, void* codes, float* scale, bool cosine, int M, int D,
                   hipStream_t s) {
  if (!sim_topk8_supported(D)) throw std::invalid_argument("gallery_pack8: needs D % 128 == 0, 128 <= D <= 4096");
  if (dt != TensorDType::F32 && dt != TensorDType::BF16) throw std::invalid_argument("gallery_pack8: rows are fp32 or bf16");
  if (M < 0) throw std::invalid_argument("gallery_pack8: M < 0");
  if (M == 0) return;
  if (!rows || !codes || !scale || (((uintptr_t)rows | (uintptr_t)codes) & 15))
    throw std::invalid_argument("gallery_pack8: null / misaligned rows or codes (16 B) or null scale");
  if (dt == TensorDType::BF16)
    hipLaunchKernelGGL(gallery_pack8_kernel<true>, dim3((M + 3) / 4), dim3(256), 0, s, rows, (uint8_t*)codes, scale, M,
                       D, cosine);
  else
    hipLaunchKernelGGL(gallery_pack8_kernel<false>, dim3((M + 3) / 4), dim3(256), 0, s, rows, (uint8_t*)codes, scale, M,
                       D, cosine);
  DMLC_HIP_CHECK(hipGetLastError());
}

void sim_topk8(const void* q, TensorDType qdt, const void* g_codes, const float* g_scale, bool cosine, int B, long N,
               int D, int k, int32_t* idx, float* score, void* ws, size_t ws_bytes, int num_cus, hipStream_t s,
               int slices_override, const int32_t* g_label, const int32_t* q_want) {
  if (!sim_topk8_supported(D)) throw std::invalid_argument("sim_topk8: needs D % 128 == 0, 128 <= D <= 4096");
  if (qdt != TensorDType::F32 && qdt != TensorDType::BF16) throw std::invalid_argument("sim_topk8: queries are fp32 or bf16");
  if (B < 0) throw std::invalid_argument("sim_topk8: B < 0");
  if (N < 1 || N > INT_MAX) throw std::invalid_argument("sim_topk8: N outside 1..2^31 - 1");
  if (k < 1 || k > N || k > kMaxTopK) throw std::invalid_argument("sim_topk8: k must be in 1..min(N, kMaxTopK)");
  if (q_want && !g_label) throw std::invalid_argument("sim_topk8: q_want needs g_label");
  if (B == 0) return;
  if (!q || !g_codes || !g_scale || !idx || !score || !ws ||
      (((uintptr_t)q | (uintptr_t)g_codes | (uintptr_t)ws) & 15))
    throw std::invalid_argument("sim_topk8: null / misaligned operand (q, g_codes and ws need 16 B; g_scale is required)");
  const int slices = slices_override ? slices_override : sim_topk_slices(B, N, num_cus);
  if (slices < 1 || slices > sim_topk_max_slices(N))
    throw std::invalid_argument("sim_topk8: slices outside 1..min(tiles, 512)");
  if (ws_bytes < sim_topk8_ws_bytes(B, k, slices)) throw std::invalid_argument("sim_topk8: workspace too small");
  const size_t cand = align256((size_t)slices * B * k * 4);
  float* cs = (float*)ws;
  int32_t* ci = (int32_t*)((char*)ws + cand);
  // the queries' codes [B][D] and scales [B], where the bf16 search keeps its packed queries
  uint8_t* qc = (uint8_t*)ws + 2 * cand;
  float* qs = (float*)(qc + (size_t)B * kMaxD);
  gallery_pack8(q, qdt, qc, qs, cosine, B, D, s);
  launch_search<true>(qc, qs, (const uint8_t*)g_codes, g_scale, B, N, D, k, idx, score, cs, ci, slices, g_label, q_want,
                      s);
}

}  // namespace dmlc
