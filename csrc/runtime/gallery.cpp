#include "gallery.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace dmlc {

Gallery::Gallery(int dim, long capacity, int device, bool cosine, int max_batch, GalleryDType dtype)
    : dim_(dim), device_(device), max_batch_(max_batch), capacity_(capacity), cosine_(cosine), dtype_(dtype) {
  const bool e4m3 = dtype_ == GalleryDType::E4M3;
  if (e4m3 && !sim_topk8_supported(dim))
    throw std::invalid_argument("Gallery: an e4m3 gallery needs dim % 128 == 0, 128 <= dim <= 4096");
  if (!sim_topk_supported(dim)) throw std::invalid_argument("Gallery: dim needs dim % 32 == 0, 32 <= dim <= 4096");
  if (capacity < 1 || capacity > INT32_MAX) throw std::invalid_argument("Gallery: capacity outside 1..2^31 - 1");
  if (max_batch < 1) throw std::invalid_argument("Gallery: max_batch < 1");
  DMLC_HIP_CHECK(hipSetDevice(device_));
  hipDeviceProp_t prop;
  DMLC_HIP_CHECK(hipGetDeviceProperties(&prop, device_));
  num_cus_ = prop.multiProcessorCount;
  // the widest launch a search can make: the slice count never exceeds the CU count
  const int slices = sim_topk_slices(max_batch_, capacity_, num_cus_);
  ws_bytes_ = e4m3 ? sim_topk8_ws_bytes(max_batch_, kMaxTopK, slices) : sim_topk_ws_bytes(max_batch_, kMaxTopK, slices);
  removed_.assign((size_t)(capacity_ + 63) / 64, 0);
  try {
    DMLC_HIP_CHECK(hipMalloc(&rows_, (size_t)capacity_ * dim_ * (e4m3 ? 1 : 2)));
    DMLC_HIP_CHECK(hipMalloc(&ws_, ws_bytes_));
    DMLC_HIP_CHECK(hipMalloc(&labels_, (size_t)capacity_ * sizeof(int32_t)));
    DMLC_HIP_CHECK(hipMalloc(&cls_idx_, (size_t)max_batch_ * kMaxTopK * sizeof(int32_t)));
    DMLC_HIP_CHECK(hipMalloc(&cls_score_, (size_t)max_batch_ * kMaxTopK * sizeof(float)));
    DMLC_HIP_CHECK(hipMalloc(&ids_dev_, (size_t)kIdsChunk * sizeof(int32_t)));
    DMLC_HIP_CHECK(hipHostMalloc(&ids_host_, (size_t)kIdsChunk * sizeof(int32_t), hipHostMallocDefault));
    if (e4m3) {  // (the queries' codes and scales live in the workspace)
      DMLC_HIP_CHECK(hipMalloc(&inv_norm_, (size_t)capacity_ * sizeof(float)));
    } else if (cosine_) {
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
  for (void* p : {rows_, (void*)inv_norm_, qpack_, (void*)q_scale_, ws_, (void*)labels_, (void*)cls_idx_,
                  (void*)cls_score_, (void*)ids_dev_})
    if (p) hipFree(p);
  if (ids_host_) hipHostFree(ids_host_);
  rows_ = qpack_ = ws_ = nullptr;
  inv_norm_ = q_scale_ = cls_score_ = nullptr;
  labels_ = cls_idx_ = ids_dev_ = ids_host_ = nullptr;
}

void Gallery::clear() {
  size_ = 0;
  removed_count_ = 0;
  std::fill(removed_.begin(), removed_.end(), 0);
}

long Gallery::add(const float* rows_dev, int M, const int32_t* labels_dev, hipStream_t s) {
  if (M < 0) throw std::invalid_argument("Gallery::add: M < 0");
  if (size_ + M > capacity_)
    throw std::invalid_argument("Gallery::add: " + std::to_string(size_) + " + " + std::to_string(M) +
                                " rows exceed the capacity " + std::to_string(capacity_));
  const long first = size_;
  if (M == 0) return first;
  DMLC_HIP_CHECK(hipSetDevice(device_));
  if (dtype_ == GalleryDType::E4M3)
    gallery_pack8(rows_dev, TensorDType::F32, (char*)rows_ + (size_t)first * dim_, inv_norm_ + first, cosine_, M, dim_, s);
  else
    gallery_pack(rows_dev, (char*)rows_ + (size_t)first * dim_ * 2, cosine_ ? inv_norm_ + first : nullptr, M, dim_, s);
  if (labels_dev)
    DMLC_HIP_CHECK(hipMemcpyAsync(labels_ + first, labels_dev, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  else
    DMLC_HIP_CHECK(hipMemsetAsync(labels_ + first, 0, (size_t)M * sizeof(int32_t), s));
  size_ += M;
  return first;
}

void Gallery::remove(const long* ids, long M, hipStream_t s) {
  if (M < 0 || (M > 0 && !ids)) throw std::invalid_argument("Gallery::remove: bad id list");
  for (long i = 0; i < M; ++i)
    if (ids[i] < 0 || ids[i] >= size_)
      throw std::invalid_argument("Gallery::remove: id " + std::to_string(ids[i]) + " outside 0.." +
                                  std::to_string(size_ - 1));
  if (M == 0) return;
  DMLC_HIP_CHECK(hipSetDevice(device_));
  for (long i0 = 0; i0 < M; i0 += kIdsChunk) {
    const int m = (int)std::min<long>(kIdsChunk, M - i0);
    for (int i = 0; i < m; ++i) ids_host_[i] = (int32_t)ids[i0 + i];
    DMLC_HIP_CHECK(hipMemcpyAsync(ids_dev_, ids_host_, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, s));
    gallery_unlabel(labels_, ids_dev_, m, size_, s);
    // the staging buffers are free again: the next chunk, or the next call, may overwrite them
    DMLC_HIP_CHECK(hipStreamSynchronize(s));
  }
  for (long i = 0; i < M; ++i) {
    uint64_t& w = removed_[(size_t)ids[i] >> 6];
    const uint64_t bit = 1ull << (ids[i] & 63);
    if (!(w & bit)) {
      w |= bit;
      ++removed_count_;
    }
  }
}

void Gallery::read_labels(int32_t* dst, hipStream_t s) {
  if (size_ == 0) return;
  if (!dst) throw std::invalid_argument("Gallery::read_labels: null destination");
  DMLC_HIP_CHECK(hipSetDevice(device_));
  DMLC_HIP_CHECK(hipMemcpyAsync(dst, labels_, (size_t)size_ * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
}

void Gallery::search(const void* q, TensorDType qdt, int B, int k, int32_t* idx, float* score, hipStream_t s,
                     const int32_t* q_want) {
  if (size_ == 0) throw std::invalid_argument("Gallery::search: the gallery is empty");
  if (B < 0 || B > max_batch_) throw std::invalid_argument("Gallery::search: B outside 0..max_batch");
  if (k < 1 || k > size_ || k > kMaxTopK)
    throw std::invalid_argument("Gallery::search: k = " + std::to_string(k) + " outside 1..min(size = " +
                                std::to_string(size_) + ", " + std::to_string(kMaxTopK) + ")");
  if (qdt != TensorDType::F32 && qdt != TensorDType::BF16)
    throw std::invalid_argument("Gallery::search: queries are fp32 or bf16");
  if (B == 0) return;
  DMLC_HIP_CHECK(hipSetDevice(device_));
  // the row filter only where it can change the answer: every label is >= 0 until a row is removed
  const bool filter = removed_count_ > 0 || q_want;
  if (dtype_ == GalleryDType::E4M3) {
    sim_topk8(q, qdt, rows_, inv_norm_, cosine_, B, size_, dim_, k, idx, score, ws_, ws_bytes_, num_cus_, s, 0,
              filter ? labels_ : nullptr, q_want);
    return;
  }
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
           num_cus_, s, 0, filter ? labels_ : nullptr, q_want);
}

void Gallery::classify(const void* q, TensorDType qdt, int B, int k, bool weighted, int32_t* label_out,
                       float* share_out, hipStream_t s) {
  if (B > 0 && (!label_out || !share_out)) throw std::invalid_argument("Gallery::classify: null output");
  search(q, qdt, B, k, cls_idx_, cls_score_, s);
  if (B == 0) return;
  knn_vote(cls_idx_, cls_score_, labels_, size_, B, k, weighted, label_out, share_out, s);
}

}  // namespace dmlc
