// An HBM-resident gallery of embeddings and the nearest-neighbour search
// over it (csrc/kernels/sim_topk.hip).
//
// Reference counterpart: none (the reference answers with a class name only).
// "Large read-mostly data lives in HBM" as the SDFS shards and the image cache
// do: rows are appended as bf16 (with their inverse L2 norms under the cosine
// metric), and a search streams them once through the MFMA, keeping each
// query's k best rows. Every row carries an int32 label (0 unless given);
// a removed row's label is -1, which the kernel's row filter reads: a search
// can be restricted to live rows of one label per query, and classify() is
// the search followed by the k-NN vote (csrc/kernels/knn_vote.hip).
//
// Storage is bf16 (the default) or e4m3: one byte per element and one fp32
// scale per row under either metric (kernels.h, sim_topk8's quantisation
// rule), searched on the block-scaled fp8 MFMA: half the bytes per row and
// half the MFMA cycles, for the rounding of a 3-bit mantissa. Everything
// below holds for both; "bf16-rounded" reads "quantised" for e4m3.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../kernels/kernels.h"

namespace dmlc {

enum class GalleryDType { BF16, E4M3 };

class Gallery {
 public:
  // Everything is allocated here, sized for max_batch queries and kMaxTopK:
  // bf16 rows [capacity, dim], inverse norms and labels [capacity], the
  // search and classify workspace, the staging of remove(). dim:
  // sim_topk_supported. E4M3: codes [capacity, dim] of one byte, scales
  // [capacity] under both metrics; dim: sim_topk8_supported.
  Gallery(int dim, long capacity, int device, bool cosine, int max_batch = 256,
          GalleryDType dtype = GalleryDType::BF16);
  ~Gallery();
  Gallery(const Gallery&) = delete;
  Gallery& operator=(const Gallery&) = delete;

  int dim() const { return dim_; }
  long capacity() const { return capacity_; }
  int device() const { return device_; }
  bool cosine() const { return cosine_; }
  GalleryDType dtype() const { return dtype_; }
  int max_batch() const { return max_batch_; }
  long size() const { return size_; }          // rows ever added since clear(), removed ones included
  long live() const { return size_ - removed_count_; }
  void clear();  // forgets rows, labels and removals; the next add starts at id 0

  // Append M fp32 rows [M, dim] (device memory, 16-B aligned) on stream s,
  // with their labels (int32 [M] in device memory, all >= 0: the caller
  // checks) or label 0 each; returns the first new row's id. Throws past
  // capacity.
  long add(const float* rows_dev, int M, const int32_t* labels_dev, hipStream_t s);
  long add(const float* rows_dev, int M, hipStream_t s) { return add(rows_dev, M, nullptr, s); }
  // Take rows out of every later search on s: their labels become -1. ids
  // (host memory) are checked against 0..size()-1 first: one bad id throws
  // and removes nothing. Removing a removed row is a no-op; ids are not
  // reused. Synchronises with s (not a hot path, not capturable).
  void remove(const long* ids, long M, hipStream_t s);
  // The k nearest rows of B <= max_batch queries (fp32 or bf16 [B, dim],
  // device memory, 16-B aligned): ids and scores [B, k], best first, equal
  // scores by ascending id. Dot metric: the dot product of the bf16-rounded
  // vectors; cosine: that times both inverse norms. Asynchronous on s, no
  // allocation, no synchronisation (capturable). An empty gallery or
  // k > size() throws. q_want (int32 [B], device memory, or null): query b
  // sees only rows labelled q_want[b] if that is >= 0. Once a row has been
  // removed or with q_want the search runs the kernel's filtered form: removed
  // rows win no rank, and a query with fewer than k candidates gets idx = -1,
  // score = -inf at the ranks left over. Otherwise it is the unfiltered launch.
  void search(const void* q, TensorDType qdt, int B, int k, int32_t* idx, float* score, hipStream_t s,
              const int32_t* q_want = nullptr);
  // search (any live row) into the gallery's own workspace, then knn_vote:
  // the winning label [B] and its share of the vote [B] (device memory).
  // Capturable as search is.
  void classify(const void* q, TensorDType qdt, int B, int k, bool weighted, int32_t* label_out, float* share_out,
                hipStream_t s);
  // the first size() labels (int32; -1: removed) -> dst (device memory), on s
  void read_labels(int32_t* dst, hipStream_t s);

 private:
  int dim_, device_, max_batch_, num_cus_ = 0;
  long capacity_, size_ = 0;
  bool cosine_;
  GalleryDType dtype_;
  void* rows_ = nullptr;        // bf16 or e4m3 [capacity, dim]
  float* inv_norm_ = nullptr;   // [capacity] (cosine; e4m3: the rows' scales under either metric)
  void* qpack_ = nullptr;       // bf16 [max_batch, dim] (cosine, fp32 queries)
  float* q_scale_ = nullptr;    // [max_batch] (cosine)
  void* ws_ = nullptr;
  size_t ws_bytes_ = 0;
  int32_t* labels_ = nullptr;   // [capacity]; -1: removed
  int32_t* cls_idx_ = nullptr;  // [max_batch, kMaxTopK] classify's search answer
  float* cls_score_ = nullptr;
  int32_t* ids_host_ = nullptr;  // pinned [kIdsChunk], remove()'s staging
  int32_t* ids_dev_ = nullptr;   // [kIdsChunk]
  static constexpr int kIdsChunk = 16384;
  std::vector<uint64_t> removed_;  // bit n: row n is removed
  long removed_count_ = 0;
};

}  // namespace dmlc
