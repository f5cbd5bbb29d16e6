// An HBM-resident gallery of embeddings and the nearest-neighbour search
// over it (csrc/kernels/sim_topk.hip).
//
// Reference counterpart: none (the reference answers with a class name only).
// "Large read-mostly data lives in HBM" as the SDFS shards and the image cache
// do: rows are appended as bf16 (with their inverse L2 norms under the cosine
// metric), and a search streams them once through the MFMA, keeping each
// query's k best rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../kernels/kernels.h"

namespace dmlc {

class Gallery {
 public:
  // Everything is allocated here, sized for max_batch queries and kMaxTopK:
  // bf16 rows [capacity, dim], inverse norms [capacity], the search
  // workspace. dim: sim_topk_supported.
  Gallery(int dim, long capacity, int device, bool cosine, int max_batch = 256);
  ~Gallery();
  Gallery(const Gallery&) = delete;
  Gallery& operator=(const Gallery&) = delete;

  int dim() const { return dim_; }
  long capacity() const { return capacity_; }
  int device() const { return device_; }
  bool cosine() const { return cosine_; }
  int max_batch() const { return max_batch_; }
  long size() const { return size_; }
  void clear() { size_ = 0; }

  // Append M fp32 rows [M, dim] (device memory, 16-B aligned) on stream s;
  // returns the first new row's id. Throws past capacity.
  long add(const float* rows_dev, int M, hipStream_t s);
  // The k nearest rows of B <= max_batch queries (fp32 or bf16 [B, dim],
  // device memory, 16-B aligned): ids and scores [B, k], best first, equal
  // scores by ascending id. Dot metric: the dot product of the bf16-rounded
  // vectors; cosine: that times both inverse norms. Asynchronous on s, no
  // allocation, no synchronisation (capturable). An empty gallery or
  // k > size() throws.
  void search(const void* q, TensorDType qdt, int B, int k, int32_t* idx, float* score, hipStream_t s);

 private:
  int dim_, device_, max_batch_, num_cus_ = 0;
  long capacity_, size_ = 0;
  bool cosine_;
  void* rows_ = nullptr;        // bf16 [capacity, dim]
  float* inv_norm_ = nullptr;   // [capacity] (cosine)
  void* qpack_ = nullptr;       // bf16 [max_batch, dim] (cosine, fp32 queries)
  float* q_scale_ = nullptr;    // [max_batch] (cosine)
  void* ws_ = nullptr;
  size_t ws_bytes_ = 0;
};

}  // namespace dmlc
