#include "gallery.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace dmlc {

Gallery::Gallery(int dim, long capacity, int device, bool cosine, int max_batch)
    : dim_(dim), device_(device), max_batch_(max_batch), capacity_(capacity), cosine_(cosine) {
  if (!sim_topk_supported(dim)) throw std::invalid_argument("Gallery: dim needs dim % 32 == 0, 32 <= dim <= 4096");
  if (capacity < 1 || capacity > INT32_MAX) throw std::invalid_argument("Gallery: capacity outside 1..2^31 - 1");
  if (max_batch < 1) throw std::invalid_argument("Gallery: max_batch < 1");
  DMLC_HIP_CHECK(hipSetDevice(device_));
  hipDeviceProp_t prop;
  DMLC_HIP_CHECK(hipGetDeviceProperties(&prop, device_));
  num_cus_ = prop.multiProcessorCount;
  // the widest launch a search can make: the slice count never exceeds the CU count
  ws_bytes_ = sim_topk_ws_bytes(max_batch_, kMaxTopK, sim_topk_slices(max_batch_, capacity_, num_cus_));
  try {
    DMLC_HIP_CHECK(hipMalloc(&rows_, (size_t)capacity_ * dim_ * 2));
    DMLC_HIP_CHECK(hipMalloc(&ws_, ws_bytes_));
    if (cosine_) {
      DMLC_HIP_CHECK(hipMalloc(&inv_norm_, (size_t)capacity_ * sizeof(float)));
      DMLC_HIP_CHECK(hipMalloc(&qpack_, (size_t)max_batch_ * dim_ * 2));
      DMLC_HIP_CHECK(hipMalloc(&q_scale_, (size_t)max_batch_ * sizeof(float)));
    }
  } catch (...) {
    this->~Gallery();
    throw;
  }
}

Gallery::~Gallery() {
  hipSetDevice(device_);
  for (void* p : {rows_, (void*)inv_norm_, qpack_, (void*)q_scale_, ws_})
    if (p) hipFree(p);
  rows_ = qpack_ = ws_ = nullptr;
  inv_norm_ = q_scale_ = nullptr;
}

long Gallery::add(const float* rows_dev, int M, hipStream_t s) {
  if (M < 0) throw std::invalid_argument("Gallery::add: M < 0");
  if (size_ + M > capacity_)
    throw std::invalid_argument("Gallery::add: " + std::to_string(size_) + " + " + std::to_string(M) +
                                " rows exceed the capacity " + std::to_string(capacity_));
  const long first = size_;
  if (M == 0) return first;
  DMLC_HIP_CHECK(hipSetDevice(device_));
  gallery_pack(rows_dev, (char*)rows_ + (size_t)first * dim_ * 2, cosine_ ? inv_norm_ + first : nullptr, M, dim_, s);
  size_ += M;
  return first;
}

void Gallery::search(const void* q, TensorDType qdt, int B, int k, int32_t* idx, float* score, hipStream_t s) {
  if (size_ == 0) throw std::invalid_argument("Gallery::search: the gallery is empty");
  if (B < 0 || B > max_batch_) throw std::invalid_argument("Gallery::search: B outside 0..max_batch");
  if (k < 1 || k > size_ || k > kMaxTopK)
    throw std::invalid_argument("Gallery::search: k = " + std::to_string(k) + " outside 1..min(size = " +
                                std::to_string(size_) + ", " + std::to_string(kMaxTopK) + ")");
  if (qdt != TensorDType::F32 && qdt != TensorDType::BF16)
    throw std::invalid_argument("Gallery::search: queries are fp32 or bf16");
  if (B == 0) return;
  DMLC_HIP_CHECK(hipSetDevice(device_));
  const float* q_scale = nullptr;
  if (cosine_) {  // the queries' inverse norms, of their bf16-rounded values
    if (qdt == TensorDType::F32) {
      gallery_pack((const float*)q, qpack_, q_scale_, B, dim_, s);
      q = qpack_;
      qdt = TensorDType::BF16;
    } else {
      gallery_inv_norms(q, q_scale_, B, dim_, s);
    }
    q_scale = q_scale_;
  }
  sim_topk(q, qdt, q_scale, rows_, cosine_ ? inv_norm_ : nullptr, B, size_, dim_, k, idx, score, ws_, ws_bytes_,
           num_cus_, s);
}

}  // namespace dmlc
