// Reference-side binding (goes into the SuperSLAM tree as include/NNMatcher.h): the mutual nearest-neighbour matcher of
// libsuperslam_hip as a superslam::IFeatureMatcher ("Pluggable feature matcher", include/InferenceInterfaces.h).  It drops in wherever a
// LightGlue* is passed today - StereoFrontEnd, LoopCloser - and needs no engine file: hloc's NN-mutual by default, NN-ratio /
// NN-superpoint through set_params.  Without a gate keypoints are accepted and ignored; with set_gate / set_stereo_gate (the epipolar band
// that src/StereoFrontEnd.cc:35-47 applies after matching, applied before the best and the second best are chosen) they are passed
// through.  distance = 1 - cosine, what tests/test_superpoint_cosine_matching.cc of the reference writes.
#ifndef NNMATCHER_HIP_ADAPTER_H_
#define NNMATCHER_HIP_ADAPTER_H_

#include <memory>
#include <opencv4/opencv2/opencv.hpp>
#include <vector>

#include "InferenceInterfaces.h"  // MatchResult, superslam::IFeatureMatcher (the reference's own header)
#include "Logging.h"
#include "SshipLogForward.h"   // library log callback -> SLOG_* (include/Logging.h:21-26)
#include "superslam_hip/nn_matcher.hpp"

class NNMatcher : public superslam::IFeatureMatcher {
public:
  explicit NNMatcher(int max_keypoints = 1024, float ratio_threshold = 0.f, float distance_threshold = 0.f, bool mutual_check = true)
      : impl_(max_keypoints, ratio_threshold, distance_threshold, mutual_check) { superslam_hip_adapter::install_log_forwarding(); }
  bool initialize() {
    const bool ok = impl_.initialize();
    if (!ok) SLOG_ERROR("NNMatcher(HIP): {}", impl_.last_error());
    return ok;
  }
  // <= 0 turns a test off; false for NaN or a ratio above 1 (the setting is then unchanged)
  bool set_params(float ratio_threshold, float distance_threshold, bool mutual_check) {
    const bool ok = impl_.set_params(ratio_threshold, distance_threshold, mutual_check);
    if (!ok) SLOG_ERROR("NNMatcher(HIP): {}", impl_.last_error());
    return ok;
  }
  // keypoint-window gate: dx_lo <= x0 - x1 <= dx_hi and dy_lo <= y0 - y1 <= dy_hi; false for a NaN bound or lo > hi (setting unchanged)
  bool set_gate(float dx_lo, float dx_hi, float dy_lo, float dy_hi) { return logged(impl_.set_gate(dx_lo, dx_hi, dy_lo, dy_hi)); }
  bool set_stereo_gate(float min_disparity, float max_disparity, float max_row_diff = 2.f) {
    return logged(impl_.set_stereo_gate(min_disparity, max_disparity, max_row_diff));
  }
  bool clear_gate() { return logged(impl_.clear_gate()); }
  bool gate_enabled() const { return impl_.gate_enabled(); }
  const float* gate() const { return impl_.gate(); }
  float ratio_threshold() const { return impl_.ratio_threshold(); }
  float distance_threshold() const { return impl_.distance_threshold(); }
  bool mutual_check() const { return impl_.mutual_check(); }

  bool match(const std::vector<cv::KeyPoint>& kp0, const cv::Mat& d0, const std::vector<cv::KeyPoint>& kp1, const cv::Mat& d1,
             MatchResult& result) {
    superslam_hip::MatchResult r;
    const bool ok = impl_.match(from_kp(kp0), from_cv(d0), from_kp(kp1), from_cv(d1), r);
    to_cv(r, result);
    return ok;
  }
  MatchResult match(const std::vector<cv::KeyPoint>& kp0, const cv::Mat& d0, const std::vector<cv::KeyPoint>& kp1,
                    const cv::Mat& d1) override {
    MatchResult r;
    match(kp0, d0, kp1, d1, r);
    return r;
  }
  MatchResult match(const std::vector<cv::KeyPoint>& kp0, const superslam::DeviceDescriptors& d0, const std::vector<cv::KeyPoint>& kp1,
                    const superslam::DeviceDescriptors& d1) override {
    MatchResult out;
    to_cv(impl_.match(from_kp(kp0), from_ref(d0), from_kp(kp1), from_ref(d1)), out);
    return out;
  }
  cv::Mat descriptors_to_host(const superslam::DeviceDescriptors& d) override {
    superslam_hip::HostDescriptors h = impl_.descriptors_to_host(from_ref(d));  // sship_desc_to_host
    return h.rows ? cv::Mat(h.rows, h.cols, CV_32F, h.data.data()).clone() : cv::Mat();
  }

private:
  bool logged(bool ok) {
    if (!ok) SLOG_ERROR("NNMatcher(HIP): {}", impl_.last_error());
    return ok;
  }
  // the keypoints are converted only while a gate is set: without one the matcher never reads them
  std::vector<superslam_hip::KeyPoint> from_kp(const std::vector<cv::KeyPoint>& kp) const {
    std::vector<superslam_hip::KeyPoint> out;
    if (!impl_.gate_enabled()) return out;
    out.resize(kp.size());
    for (size_t i = 0; i < kp.size(); ++i) { out[i].x = kp[i].pt.x; out[i].y = kp[i].pt.y; }
    return out;
  }
  static superslam_hip::HostDescriptors from_cv(const cv::Mat& m) {
    superslam_hip::HostDescriptors h;
    cv::Mat f;
    if (m.type() == CV_32F) f = m.isContinuous() ? m : m.clone(); else m.convertTo(f, CV_32F);
    h.rows = f.rows; h.cols = f.cols;
    h.data.assign(reinterpret_cast<const float*>(f.data), reinterpret_cast<const float*>(f.data) + f.total());
    return h;
  }
  static superslam_hip::DeviceDescriptors from_ref(const superslam::DeviceDescriptors& d) {
    superslam_hip::DeviceDescriptors o;
    o.data = d.data; o.count = d.count; o.dim = d.dim; o.slot = d.slot; o.slot_ref = d.slot_ref;
    return o;
  }
  static void to_cv(const superslam_hip::MatchResult& in, MatchResult& out) {
    out.matches.clear();
    for (const auto& m : in.matches) {
      cv::DMatch dm;
      dm.queryIdx = m.queryIdx; dm.trainIdx = m.trainIdx; dm.distance = m.distance;
      out.matches.push_back(dm);
    }
  }
  superslam_hip::NNMatcher impl_;
};
typedef std::shared_ptr<NNMatcher> NNMatcherPtr;
#endif
