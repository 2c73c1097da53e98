// superslam_hip/nn_matcher.hpp - the mutual nearest-neighbour matcher (include/sship.h "Nearest-neighbour matcher") as a second
// IFeatureMatcher next to superslam_hip::LightGlue (frontend.hpp): hloc's NN-mutual / NN-ratio / NN-superpoint.  Same method shapes as
// LightGlue, so it plugs in wherever a matcher is passed; no weights and no image size.  Keypoints are accepted for interface parity
// and ignored: the set sizes are the descriptor counts.  Results go through sship_filter_matches (distance = 1 - cosine).
#pragma once
#include "frontend.hpp"

namespace superslam_hip {

class NNMatcher : public IFeatureMatcher {
public:
  explicit NNMatcher(int max_keypoints = 1024, float ratio_threshold = 0.f, float distance_threshold = 0.f, bool mutual_check = true)
      : max_keypoints_(max_keypoints), ratio_(ratio_threshold), dist_(distance_threshold), mutual_(mutual_check) {}
  ~NNMatcher() override { if (nn_) sship_nn_destroy(nn_); }
  NNMatcher(const NNMatcher&) = delete;
  NNMatcher& operator=(const NNMatcher&) = delete;

  bool initialize() {
    if (nn_) return true;
    if (!valid(ratio_, dist_)) { last_error_ = "NNMatcher: ratio_threshold must be <= 1 and neither threshold NaN"; return false; }
    if (sship_nn_create(max_keypoints_, 1, &nn_) != SSHIP_OK) { last_error_ = sship_last_error(); nn_ = nullptr; return false; }
    if (sship_nn_set_params(nn_, ratio_, dist_, mutual_ ? 1 : 0) != SSHIP_OK) {
      last_error_ = sship_last_error(); sship_nn_destroy(nn_); nn_ = nullptr; return false;
    }
    return true;
  }
  // <= 0 turns a test off.  Before initialize() the values are kept and applied there; after it, they apply to the next match.
  // false (last_error()) for NaN or a ratio above 1; the setting is then unchanged.
  bool set_params(float ratio_threshold, float distance_threshold, bool mutual_check) {
    if (nn_ && sship_nn_set_params(nn_, ratio_threshold, distance_threshold, mutual_check ? 1 : 0) != SSHIP_OK) {
      last_error_ = sship_last_error(); return false;
    }
    if (!nn_ && !valid(ratio_threshold, distance_threshold)) {
      last_error_ = "set_params: ratio_threshold must be <= 1 and neither threshold NaN"; return false;
    }
    ratio_ = ratio_threshold; dist_ = distance_threshold; mutual_ = mutual_check;
    return true;
  }
  float ratio_threshold() const { return ratio_; }
  float distance_threshold() const { return dist_; }
  bool mutual_check() const { return mutual_; }

  // 5-argument form, as LightGlue's: false for an uninitialised matcher or an empty set.
  bool match(const std::vector<KeyPoint>&, const HostDescriptors& d0, const std::vector<KeyPoint>&, const HostDescriptors& d1,
             MatchResult& result) {
    result.matches.clear();
    if (!nn_ || d0.rows <= 0 || d1.rows <= 0 || d0.cols != SSHIP_DESC_DIM || d1.cols != SSHIP_DESC_DIM) return false;
    std::vector<int32_t> m0(d0.rows);
    std::vector<float> ms0(d0.rows);
    if (sship_nn_match_host(nn_, d0.rows, d0.data.data(), d1.rows, d1.data.data(), m0.data(), ms0.data()) != SSHIP_OK) {
      last_error_ = sship_last_error(); return false;
    }
    postprocess(m0, ms0, result);
    return true;
  }
  MatchResult match(const std::vector<KeyPoint>& kp0, const HostDescriptors& d0, const std::vector<KeyPoint>& kp1,
                    const HostDescriptors& d1) override {
    MatchResult r;
    match(kp0, d0, kp1, d1, r);
    return r;
  }
  MatchResult match(const std::vector<KeyPoint>&, const DeviceDescriptors& d0, const std::vector<KeyPoint>&,
                    const DeviceDescriptors& d1) override {
    MatchResult r;
    if (!nn_ || d0.empty() || d1.empty()) return r;
    std::vector<int32_t> m0(d0.count);
    std::vector<float> ms0(d0.count);
    if (sship_nn_match_device(nn_, d0.count, d0.data, d1.count, d1.data, m0.data(), ms0.data()) != SSHIP_OK) {
      last_error_ = sship_last_error(); return r;
    }
    postprocess(m0, ms0, r);
    return r;
  }
  HostDescriptors descriptors_to_host(const DeviceDescriptors& d) override {
    HostDescriptors out;
    if (d.empty()) return out;
    out.data.resize(static_cast<size_t>(d.count) * d.dim);
    if (sship_desc_to_host(d.data, d.count, d.dim, out.data.data()) != SSHIP_OK) { last_error_ = sship_last_error(); return HostDescriptors(); }
    out.rows = d.count; out.cols = d.dim;
    return out;
  }
  const std::string& last_error() const { return last_error_; }
  sship_nn* handle() const { return nn_; }

private:
  static bool valid(float r, float t) { return r <= 1.f && t == t; }  // r <= 1 is false for NaN
  static void postprocess(const std::vector<int32_t>& m0, const std::vector<float>& ms0, MatchResult& r) {
    const int n0 = static_cast<int>(m0.size());
    std::vector<int> q(n0), t(n0);
    std::vector<float> dist(n0);
    const int k = sship_filter_matches(m0.data(), ms0.data(), n0, q.data(), t.data(), dist.data());
    for (int i = 0; i < k; ++i) { DMatch dm; dm.queryIdx = q[i]; dm.trainIdx = t[i]; dm.distance = dist[i]; r.matches.push_back(dm); }
  }
  int max_keypoints_;
  float ratio_, dist_;
  bool mutual_;
  sship_nn* nn_ = nullptr;
  std::string last_error_;
};
typedef std::shared_ptr<NNMatcher> NNMatcherPtr;

}  // namespace superslam_hip
