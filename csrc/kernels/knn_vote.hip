// k-NN vote: from a nearest-neighbour search's answer (sim_topk.hip) and the
// gallery's labels, each query's winning label and its share of the vote.
//
// Reference counterpart: none (the reference answers with a class name only).
// What torch users write instead pulls idx / score [B, k] back, gathers the
// labels and loops (or scatter_adds into a [B, classes] matrix whose sums
// come in no fixed order).
//
// The whole rule, so that a host can replay it bit for bit:
//  * rank j votes iff 0 <= idx[b][j] < N; its label is g_label[idx[b][j]];
//  * its weight is 1 (uniform) or max(score[b][j], 0) (weighted);
//  * a label's total is the fp32 sum of its ranks' weights, added in
//    ascending rank order starting from 0;
//  * the label with the largest total wins; among equal totals the label
//    whose best (lowest) rank comes first;
//  * share = the winner's total / the fp32 sum of all voting weights in
//    ascending rank order (the IEEE divide), 0 if that sum is 0;
//  * no voter: label -1, share 0.
//
// Sixteen lanes per query, four queries a wave: lane j < k holds rank j's
// label and weight. Every lane walks the k ranks in order (one broadcast of
// label, weight and vote per rank) and sums the weights of its own label, so
// lane j ends with its label's total and that label's best rank; the
// (total, best rank) arg-max over the 16 lanes picks the winner. k <= 16
// adds a lane: nothing is worth sharing between lanes of equal labels.
#include "common.h"
#include "kernels.h"

#include <climits>

namespace dmlc {

namespace {

__global__ __launch_bounds__(256) void knn_vote_kernel(const int32_t* __restrict__ idx, const float* __restrict__ score,
                                                       const int32_t* __restrict__ g_label, long N, int B, int k,
                                                       int weighted, int32_t* __restrict__ label,
                                                       float* __restrict__ share) {
  const int j = threadIdx.x & 15;
  const int b = blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool mine = b < B && j < k;
  int n = -1;
  float w = 0.f;
  if (mine) {
    n = idx[(long)b * k + j];
    w = weighted ? fmaxf(score[(long)b * k + j], 0.f) : 1.f;
  }
  const int votes = mine && n >= 0 && n < N;
  const int lab = votes ? g_label[n] : 0;
  // this lane's label: its total and its best rank; the sum of all weights
  float tot = 0.f, all = 0.f;
  int first = INT_MAX;
  for (int i = 0; i < k; ++i) {  // (k is uniform)
    const int vi = __shfl(votes, i, 16);
    const int li = __shfl(lab, i, 16);
    const float wi = __shfl(w, i, 16);
    if (vi) {
      all += wi;
      if (li == lab) {
        tot += wi;
        first = first == INT_MAX ? i : first;
      }
    }
  }
  if (!votes) {  // weights are >= 0, so any voter beats -1
    tot = -1.f;
    first = INT_MAX;
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const float ot = __shfl_xor(tot, o, 16);
    const int of = __shfl_xor(first, o, 16);
    if (ot > tot || (ot == tot && of < first)) {
      tot = ot;
      first = of;
    }
  }
  const int win = __shfl(lab, first == INT_MAX ? 0 : first, 16);
  if (b < B && j == 0) {
    const bool any = first != INT_MAX;
    label[b] = any ? win : -1;
    share[b] = any && all != 0.f ? tot / all : 0.f;
  }
}

}  // namespace

void knn_vote(const int32_t* idx, const float* score, const int32_t* g_label, long N, int B, int k, bool weighted,
              int32_t* label, float* share, hipStream_t s) {
  if (B < 0) throw std::invalid_argument("knn_vote: B < 0");
  if (k < 1 || k > kMaxTopK) throw std::invalid_argument("knn_vote: k outside 1..kMaxTopK");
  if (N < 1 || N > INT_MAX) throw std::invalid_argument("knn_vote: N outside 1..2^31 - 1");
  if (B == 0) return;
  if (!idx || !score || !g_label || !label || !share) throw std::invalid_argument("knn_vote: null operand");
  hipLaunchKernelGGL(knn_vote_kernel, dim3((B + 15) / 16), dim3(256), 0, s, idx, score, g_label, N, B, k,
                     (int)weighted, label, share);
  DMLC_HIP_CHECK(hipGetLastError());
}

}  // namespace dmlc
