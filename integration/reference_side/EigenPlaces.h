// Reference-side binding (goes into the SuperSLAM tree as include/EigenPlaces.h; replaces the TensorRT runner).
// Same class name, constructor and methods as the reference's header (include/EigenPlaces.h:19-40): SuperSLAM.cc:116-133 and
// LoopCloser compile and run unchanged against superslam::IPlaceRecognizer.  The descriptor is computed by libsuperslam_hip.so
// (include/superslam_hip/place_recognizer.hpp -> include/sship.h, sship_ep_*); retrieval stays the reference's own
// superslam::CosineDescriptorIndex (src/PlaceRecognizer.cc in libsuperslam_core), held and used exactly as include/EigenPlaces.h:30-36,53,62.
// Opt-in: set_device_index(true, capacity) moves retrieval to the device-resident index of the library
// (include/superslam_hip/place_index.hpp -> sship_index_*: the same rule, ties by insertion order, topK <= 0 refused); off by default.
#ifndef EIGENPLACES_HIP_ADAPTER_H_
#define EIGENPLACES_HIP_ADAPTER_H_

#include <cstdlib>
#include <memory>
#include <opencv4/opencv2/core.hpp>
#include <string>
#include <vector>

#include "Logging.h"
#include "SshipLogForward.h"   // library log callback -> SLOG_* (include/Logging.h:21-26)
#include "PlaceRecognizer.h"  // the reference's own header (unchanged): superslam::IPlaceRecognizer, LoopCandidate
#include "superslam_hip/place_index.hpp"
#include "superslam_hip/place_recognizer.hpp"

class EigenPlaces : public superslam::IPlaceRecognizer {
public:
  EigenPlaces(const std::string& engine_file, int input_width, int input_height) : impl_(engine_file, input_width, input_height) {
    superslam_hip_adapter::install_log_forwarding();
    if (const char* s = std::getenv("SUPERSLAM_LOOP_MIN_SCORE")) min_score_ = static_cast<float>(std::atof(s));  // src/EigenPlaces.cc:33-34
  }
  bool initialize() {
    const bool ok = impl_.initialize();
    if (!ok) SLOG_ERROR("EigenPlaces(HIP): {}", impl_.last_error());
    return ok;
  }
  cv::Mat compute_global_descriptor(const cv::Mat& image) override {
    cv::Mat keep = image.isContinuous() ? image : image.clone();
    if (keep.depth() != CV_8U) keep.convertTo(keep, CV_8U);
    const superslam_hip::GlobalDescriptor d = impl_.compute_global_descriptor(
        superslam_hip::Image{keep.data, keep.rows, keep.cols, keep.channels(), static_cast<int>(keep.step)});
    if (d.empty()) return cv::Mat();
    cv::Mat out(1, static_cast<int>(d.size()), CV_32F);
    for (size_t i = 0; i < d.size(); ++i) out.ptr<float>(0)[i] = d[i];
    return out;
  }
  // Batches (not part of superslam::IPlaceRecognizer): reserve_batch(n) once, then one descriptor row (1 x 512, CV_32F) per image of a
  // sequence of images of ONE size and type; row b has the bits of compute_global_descriptor(images[b]).  Empty on failure.
  bool reserve_batch(int n) {
    const bool ok = impl_.reserve_batch(n);
    if (!ok) SLOG_ERROR("EigenPlaces(HIP): {}", impl_.last_error());
    return ok;
  }
  std::vector<cv::Mat> compute_global_descriptors(const std::vector<cv::Mat>& images) {
    std::vector<cv::Mat> keep;
    std::vector<superslam_hip::Image> views;
    for (const cv::Mat& image : images) {
      cv::Mat k = image.isContinuous() ? image : image.clone();
      if (k.depth() != CV_8U) k.convertTo(k, CV_8U);
      keep.push_back(k);
    }
    for (const cv::Mat& k : keep) views.push_back(superslam_hip::Image{k.data, k.rows, k.cols, k.channels(), static_cast<int>(k.step)});
    const std::vector<superslam_hip::GlobalDescriptor> ds = impl_.compute_global_descriptors(views);
    if (ds.size() != images.size() && !images.empty()) SLOG_ERROR("EigenPlaces(HIP): {}", impl_.last_error());
    std::vector<cv::Mat> out;
    for (const auto& d : ds) {
      cv::Mat row(1, static_cast<int>(d.size()), CV_32F);
      for (size_t i = 0; i < d.size(); ++i) row.ptr<float>(0)[i] = d[i];
      out.push_back(row);
    }
    return out;
  }
  // Retrieval on the device (default off).  Switch before the first add: the two indices do not share their content, and a switch
  // starts from an empty device index of `capacity` rows.
  void set_device_index(bool on, int capacity = 16384) {
    device_index_.reset(on ? new superslam_hip::DescriptorIndex(capacity) : nullptr);
  }
  bool device_index() const { return device_index_ != nullptr; }
  void add(size_t keyframe_id, const cv::Mat& global_descriptor) override {
    if (!device_index_) { index_.add(keyframe_id, global_descriptor); return; }
    const cv::Mat row = float_row(global_descriptor);
    if (!device_index_->add(keyframe_id, row.ptr<float>(0), row.cols)) SLOG_ERROR("EigenPlaces(HIP) index: {}", device_index_->last_error());
  }
  std::vector<superslam::LoopCandidate> query(const cv::Mat& global_descriptor, size_t excludeRecent, int topK) override {
    if (!device_index_) return index_.query(global_descriptor, excludeRecent, topK, min_score_);
    std::vector<superslam::LoopCandidate> out;
    if (device_index_->size() == 0) return out;
    const cv::Mat row = float_row(global_descriptor);
    const auto found = device_index_->query(row.ptr<float>(0), row.cols, excludeRecent, topK, min_score_);
    if (found.empty() && !device_index_->last_error().empty()) SLOG_ERROR("EigenPlaces(HIP) index: {}", device_index_->last_error());
    for (const auto& c : found) { superslam::LoopCandidate lc; lc.keyframe_id = c.keyframe_id; lc.score = c.score; out.push_back(lc); }
    return out;
  }

private:
  static cv::Mat float_row(const cv::Mat& desc) {  // normalizedRow's first half (src/PlaceRecognizer.cc:10-13): 1 x D, CV_32F
    cv::Mat row = desc.reshape(1, 1);
    if (row.type() != CV_32F) row.convertTo(row, CV_32F);
    return row;
  }
  superslam_hip::EigenPlaces impl_;
  float min_score_ = 0.75f;                  // include/EigenPlaces.h:53
  superslam::CosineDescriptorIndex index_;   // include/EigenPlaces.h:62
  std::unique_ptr<superslam_hip::DescriptorIndex> device_index_;   // set_device_index(true): retrieval on the device instead
};
#endif
