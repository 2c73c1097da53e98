// superslam_hip/place_index.hpp - the device-resident retrieval side of the place recogniser (include/sship.h "Place-recognition index"):
// superslam_hip::DescriptorIndex mirrors the reference's superslam::CosineDescriptorIndex (include/PlaceRecognizer.h,
// src/PlaceRecognizer.cc:21-52) over the C ABI (sship_index_*).  Same methods - add(id, descriptor), query(descriptor, excludeRecent, topK,
// minScore) -> candidates best first, size() - with a descriptor as (const float*, dim) where the reference has a cv::Mat.  The capacity
// is given at construction; the dimension is fixed by the first add (the handle is created there).  A failed call returns false / an
// empty result, never throws, and records last_error().  One stated difference from the reference: topK <= 0 ("all") is refused.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../sship.h"

namespace superslam_hip {

class DescriptorIndex {
public:
  struct Candidate {
    size_t keyframe_id;
    float score;
  };
  explicit DescriptorIndex(int capacity = 16384, int max_top_k = 50) : capacity_(capacity), max_top_k_(max_top_k) {}
  ~DescriptorIndex() { if (ix_) sship_index_destroy(ix_); }
  DescriptorIndex(const DescriptorIndex&) = delete;
  DescriptorIndex& operator=(const DescriptorIndex&) = delete;

  // CosineDescriptorIndex::add.  false (last_error()) for a null / mis-sized descriptor, a full index or a run-time failure.
  bool add(size_t keyframe_id, const float* descriptor, int dim) {
    if (!descriptor) { last_error_ = "DescriptorIndex::add: null descriptor"; return false; }
    if (!ensure(dim, "add")) return false;
    const int64_t id = static_cast<int64_t>(keyframe_id);
    if (sship_index_add_host(ix_, &id, descriptor, 1, dim) != SSHIP_OK) { last_error_ = sship_last_error(); return false; }
    return true;
  }
  bool add(size_t keyframe_id, const std::vector<float>& descriptor) { return add(keyframe_id, descriptor.data(), static_cast<int>(descriptor.size())); }
  // the descriptor is already on the device (what sship_ep_infer_u8_device wrote); asynchronous on `stream`
  bool add_device(size_t keyframe_id, const float* descriptor_dev, int dim, void* stream = nullptr) {
    if (!descriptor_dev) { last_error_ = "DescriptorIndex::add_device: null descriptor"; return false; }
    if (!ensure(dim, "add_device")) return false;
    const int64_t id = static_cast<int64_t>(keyframe_id);
    if (sship_index_add_device(ix_, &id, descriptor_dev, 1, dim, stream) != SSHIP_OK) { last_error_ = sship_last_error(); return false; }
    return true;
  }
  // CosineDescriptorIndex::query: rows older than the excludeRecent newest, score >= minScore, best first, at most topK.
  std::vector<Candidate> query(const float* descriptor, int dim, size_t excludeRecent, int topK, float minScore) {
    std::vector<Candidate> out;
    if (!check_query(descriptor, dim, topK, minScore, "query")) return out;
    if (!ix_) return out;  // nothing added yet: the reference returns an empty list
    return finish(sship_index_query_host(ix_, descriptor, clamp_recent(excludeRecent), topK, minScore, ids_.data(), scores_.data(), &count_));
  }
  std::vector<Candidate> query(const std::vector<float>& descriptor, size_t excludeRecent, int topK, float minScore) {
    return query(descriptor.data(), static_cast<int>(descriptor.size()), excludeRecent, topK, minScore);
  }
  std::vector<Candidate> query_device(const float* descriptor_dev, int dim, size_t excludeRecent, int topK, float minScore) {
    std::vector<Candidate> out;
    if (!check_query(descriptor_dev, dim, topK, minScore, "query_device")) return out;
    if (!ix_) return out;
    return finish(sship_index_query_device(ix_, descriptor_dev, clamp_recent(excludeRecent), topK, minScore, ids_.data(), scores_.data(), &count_));
  }
  size_t size() const { return static_cast<size_t>(sship_index_size(ix_)); }
  int dim() const { return dim_; }
  int capacity() const { return capacity_; }
  void clear() { if (ix_) sship_index_clear(ix_); }
  const std::string& last_error() const { return last_error_; }
  sship_index* handle() const { return ix_; }

private:
  bool ensure(int dim, const char* who) {
    if (ix_) {
      if (dim != dim_) { last_error_ = std::string("DescriptorIndex::") + who + ": the dimension was fixed by the first add"; return false; }
      return true;
    }
    if (sship_index_create(dim, capacity_, 1, max_top_k_, &ix_) != SSHIP_OK) { last_error_ = sship_last_error(); ix_ = nullptr; return false; }
    dim_ = dim;
    ids_.resize(static_cast<size_t>(max_top_k_));
    scores_.resize(static_cast<size_t>(max_top_k_));
    return true;
  }
  bool check_query(const float* descriptor, int dim, int topK, float minScore, const char* who) {
    if (!descriptor) { last_error_ = std::string("DescriptorIndex::") + who + ": null descriptor"; return false; }
    if (topK < 1 || topK > max_top_k_) { last_error_ = std::string("DescriptorIndex::") + who + ": topK must be in [1, max_top_k] (there is no 'all')"; return false; }
    if (minScore != minScore) { last_error_ = std::string("DescriptorIndex::") + who + ": minScore is NaN"; return false; }
    if (ix_ && dim != dim_) { last_error_ = std::string("DescriptorIndex::") + who + ": the dimension was fixed by the first add"; return false; }
    return true;
  }
  static int clamp_recent(size_t excludeRecent) { return excludeRecent > 0x7fffffffu ? 0x7fffffff : static_cast<int>(excludeRecent); }
  std::vector<Candidate> finish(int rc) {
    std::vector<Candidate> out;
    if (rc != SSHIP_OK) { last_error_ = sship_last_error(); return out; }
    out.reserve(static_cast<size_t>(count_));
    for (int i = 0; i < count_; ++i) out.push_back(Candidate{static_cast<size_t>(ids_[static_cast<size_t>(i)]), scores_[static_cast<size_t>(i)]});
    return out;
  }
  int capacity_, max_top_k_;
  int dim_ = 0, count_ = 0;
  sship_index* ix_ = nullptr;
  std::vector<int64_t> ids_;
  std::vector<float> scores_;
  std::string last_error_;
};

}  // namespace superslam_hip
