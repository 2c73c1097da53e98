// superslam_hip/nn_matcher.hpp - the mutual nearest-neighbour matcher (include/sship.h "Nearest-neighbour matcher") as a second
// IFeatureMatcher next to superslam_hip::LightGlue (frontend.hpp): hloc's NN-mutual / NN-ratio / NN-superpoint.  Same method shapes as
// LightGlue, so it plugs in wherever a matcher is passed; no weights and no image size.  Without a gate keypoints are accepted for
// interface parity and ignored: the set sizes are the descriptor counts.  With a keypoint-window gate (include/sship.h "Keypoint-window
// gate": set_gate / set_stereo_gate / clear_gate) the matches pass their keypoints through and an entry outside the window is absent
// from the search.  Results go through sship_filter_matches (distance = 1 - cosine).
#pragma once
#include <cmath>

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
    if (sship_nn_set_params(nn_, ratio_, dist_, mutual_ ? 1 : 0) != SSHIP_OK ||
        sship_nn_set_gate(nn_, gate_on_ ? 1 : 0, gate_[0], gate_[1], gate_[2], gate_[3]) != SSHIP_OK) {
      last_error_ = sship_last_error(); sship_nn_destroy(nn_); nn_ = nullptr; return false;
    }
    return true;
  }
  // The keypoint-window gate: an entry is present only if dx_lo <= x0 - x1 <= dx_hi and dy_lo <= y0 - y1 <= dy_hi (bounds may be
  // +-INFINITY).  Before initialize() the gate is kept and applied there.  false (last_error()) for a NaN bound or lo > hi; the setting is
  // then unchanged.
  bool set_gate(float dx_lo, float dx_hi, float dy_lo, float dy_hi) { return apply_gate(true, dx_lo, dx_hi, dy_lo, dy_hi); }
  // rectified stereo: min_disparity <= uL - uR <= max_disparity and |vL - vR| <= max_row_diff
  bool set_stereo_gate(float min_disparity, float max_disparity, float max_row_diff = 2.f) {
    return apply_gate(true, min_disparity, max_disparity, -max_row_diff, max_row_diff);
  }
  bool clear_gate() { return apply_gate(false, -INFINITY, INFINITY, -INFINITY, INFINITY); }
  bool gate_enabled() const { return gate_on_; }
  const float* gate() const { return gate_; }  // (dx_lo, dx_hi, dy_lo, dy_hi)
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
  bool match(const std::vector<KeyPoint>& kp0, const HostDescriptors& d0, const std::vector<KeyPoint>& kp1, const HostDescriptors& d1,
             MatchResult& result) {
    result.matches.clear();
    if (!nn_ || d0.rows <= 0 || d1.rows <= 0 || d0.cols != SSHIP_DESC_DIM || d1.cols != SSHIP_DESC_DIM) return false;
    std::vector<int32_t> m0(d0.rows);
    std::vector<float> ms0(d0.rows);
    int rc;
    if (gate_on_) {
      std::vector<float> k0, k1;
      if (!flatten(kp0, d0.rows, k0) || !flatten(kp1, d1.rows, k1)) return false;
      rc = sship_nn_match_gated_host(nn_, k0.data(), 2, d0.rows, d0.data.data(), k1.data(), 2, d1.rows, d1.data.data(), m0.data(), ms0.data());
    } else {
      rc = sship_nn_match_host(nn_, d0.rows, d0.data.data(), d1.rows, d1.data.data(), m0.data(), ms0.data());
    }
    if (rc != SSHIP_OK) {
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
  MatchResult match(const std::vector<KeyPoint>& kp0, const DeviceDescriptors& d0, const std::vector<KeyPoint>& kp1,
                    const DeviceDescriptors& d1) override {
    MatchResult r;
    if (!nn_ || d0.empty() || d1.empty()) return r;
    std::vector<int32_t> m0(d0.count);
    std::vector<float> ms0(d0.count);
    int rc;
    if (gate_on_) {
      std::vector<float> k0, k1;
      if (!flatten(kp0, d0.count, k0) || !flatten(kp1, d1.count, k1)) return r;
      rc = sship_nn_match_gated_device(nn_, k0.data(), 2, d0.count, d0.data, k1.data(), 2, d1.count, d1.data, m0.data(), ms0.data());
    } else {
      rc = sship_nn_match_device(nn_, d0.count, d0.data, d1.count, d1.data, m0.data(), ms0.data());
    }
    if (rc != SSHIP_OK) {
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
  bool apply_gate(bool on, float dx_lo, float dx_hi, float dy_lo, float dy_hi) {
    if (nn_ && sship_nn_set_gate(nn_, on ? 1 : 0, dx_lo, dx_hi, dy_lo, dy_hi) != SSHIP_OK) { last_error_ = sship_last_error(); return false; }
    if (!nn_ && !(dx_lo <= dx_hi && dy_lo <= dy_hi)) {  // false for NaN too
      last_error_ = "set_gate: bounds must satisfy lo <= hi and none may be NaN"; return false;
    }
    gate_on_ = on; gate_[0] = dx_lo; gate_[1] = dx_hi; gate_[2] = dy_lo; gate_[3] = dy_hi;
    return true;
  }
  // the gated calls read (x, y) of exactly one keypoint per descriptor row
  bool flatten(const std::vector<KeyPoint>& kp, int n, std::vector<float>& out) {
    if (static_cast<int>(kp.size()) != n) { last_error_ = "NNMatcher: a gate is set and the keypoint count differs from the descriptor count"; return false; }
    out.resize(static_cast<size_t>(n) * 2);
    for (int i = 0; i < n; ++i) { out[2 * i] = kp[i].x; out[2 * i + 1] = kp[i].y; }
    return true;
  }
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
  bool gate_on_ = false;
  float gate_[4] = {-INFINITY, INFINITY, -INFINITY, INFINITY};
  sship_nn* nn_ = nullptr;
  std::string last_error_;
};
typedef std::shared_ptr<NNMatcher> NNMatcherPtr;

}  // namespace superslam_hip
