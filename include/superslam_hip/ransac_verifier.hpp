// superslam_hip/ransac_verifier.hpp - the RANSAC pose seed and inlier gate above the C ABI (include/sship.h "RANSAC pose seed and inlier
// gate"): superslam_hip::RansacVerifier::verify(observations) finds the pose and the inlier set of one pair when the seed is unknown and
// many matches are wrong - the step in front of PoseSolver::track in LoopCloser::verify (src/LoopCloser.cc:55-89) and in front of the
// observations handed to WindowSmoother::add_keyframe.  Observations and poses are pose_solver.hpp's (StereoPointObs, Pose3x4: Twc,
// row-major [R | t]); the solver reads fp32, so the values are narrowed once on the way in.  The rule is the library's own (sship.h).
// The handle is created by the first call.  A failed call returns ok = false with the identity, never throws, and records last_error().
// Bad arguments (camera, parameters, more observations than max_obs) are refused without touching a device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../sship.h"
#include "pose_solver.hpp"

namespace superslam_hip {

class RansacVerifier {
public:
  struct Result {
    bool ok = false;
    Pose3x4 pose{};
    int n_present = 0, n_inliers = 0, best_h = -1, status = SSHIP_RANSAC_TOO_FEW;
    double cost = 0.0;
  };
  static sship_ransac_params default_params() { return sship_ransac_params{3.0, 1.0, 1e-8, 1u, 512}; }

  explicit RansacVerifier(const StereoCalibration& K, int max_obs = 2048) : K_(K), max_obs_(max_obs), params_(default_params()) {}
  ~RansacVerifier() { if (rs_) sship_ransac_destroy(rs_); }
  RansacVerifier(const RansacVerifier&) = delete;
  RansacVerifier& operator=(const RansacVerifier&) = delete;

  // the rule's constants; false (last_error()) and the old values kept for a NaN, an infinity, a negative value, a bad hypothesis count
  bool set_params(const sship_ransac_params& p) {
    if (!check_params(p)) return false;
    if (rs_ && sship_ransac_set_params(rs_, &p) != SSHIP_OK) { last_error_ = sship_last_error(); return false; }
    params_ = p;
    return true;
  }
  const sship_ransac_params& params() const { return params_; }

  // inliers (optional) receives one byte per observation: the winner's inlier mask, the gate for what is solved next
  Result verify(const std::vector<StereoPointObs>& matches, std::vector<uint8_t>* inliers = nullptr) {
    Result r;
    r.pose = PoseSolver::identity();
    const size_t n = matches.size();
    if (n > static_cast<size_t>(max_obs_ > 0 ? max_obs_ : 0)) { last_error_ = "RansacVerifier::verify: more observations than max_obs"; return r; }
    if (!ensure()) return r;
    pts_.resize(3 * n); meas_.resize(3 * n);
    for (size_t i = 0; i < n; ++i) {
      const StereoPointObs& o = matches[i];
      pts_[3 * i] = static_cast<float>(o.X); pts_[3 * i + 1] = static_cast<float>(o.Y); pts_[3 * i + 2] = static_cast<float>(o.Z);
      meas_[3 * i] = static_cast<float>(o.uL); meas_[3 * i + 1] = static_cast<float>(o.uR); meas_[3 * i + 2] = static_cast<float>(o.v);
    }
    if (inliers) inliers->assign(n, 0);
    int32_t stats[4] = {0, 0, -1, SSHIP_RANSAC_TOO_FEW};
    double cost = 0.0;
    Pose3x4 out{};
    if (sship_ransac_solve_host(rs_, pts_.data(), meas_.data(), nullptr, static_cast<int>(n), out.data(), stats, &cost,
                                inliers && n ? inliers->data() : nullptr) != SSHIP_OK) {
      last_error_ = sship_last_error();
      return r;
    }
    r.ok = true; r.pose = out;
    r.n_present = stats[0]; r.n_inliers = stats[1]; r.best_h = stats[2]; r.status = stats[3];
    r.cost = cost;
    return r;
  }
  // the chain of LoopCloser::verify: the RANSAC pose seeds `solver`, which sees the RANSAC inliers only; inliers (optional) receives the
  // solver's mask in the positions of `matches`
  PoseSolver::Result verify_and_track(PoseSolver& solver, const std::vector<StereoPointObs>& matches, std::vector<uint8_t>* inliers = nullptr,
                                      Result* seed = nullptr) {
    std::vector<uint8_t> gate;
    const Result r = verify(matches, &gate);
    if (seed) *seed = r;
    PoseSolver::Result none;
    none.pose = PoseSolver::identity();
    if (inliers) inliers->assign(matches.size(), 0);
    if (!r.ok) return none;
    std::vector<StereoPointObs> kept;
    std::vector<size_t> where;
    for (size_t i = 0; i < matches.size(); ++i)
      if (gate[i]) { kept.push_back(matches[i]); where.push_back(i); }
    std::vector<uint8_t> in;
    const PoseSolver::Result t = solver.track(r.pose, kept, inliers ? &in : nullptr);
    if (!t.ok) last_error_ = solver.last_error();
    if (inliers && t.ok)
      for (size_t k = 0; k < where.size(); ++k) (*inliers)[where[k]] = in[k];
    return t;
  }
  int max_obs() const { return max_obs_; }
  const StereoCalibration& calibration() const { return K_; }
  const std::string& last_error() const { return last_error_; }
  sship_ransac* handle() const { return rs_; }

private:
  bool check_params(const sship_ransac_params& p) {
    const double all[3] = {p.inlier_px, p.min_disparity, p.min_area2};
    for (double v : all)
      if (!std::isfinite(v)) { last_error_ = "RansacVerifier: a parameter is NaN or infinite"; return false; }
    if (p.inlier_px < 0 || p.min_disparity < 0 || p.min_area2 < 0) { last_error_ = "RansacVerifier: inlier_px, min_disparity or min_area2 is negative"; return false; }
    if (p.num_hypotheses < 1 || p.num_hypotheses > 65536) { last_error_ = "RansacVerifier: num_hypotheses must be in [1, 65536]"; return false; }
    return true;
  }
  bool ensure() {
    if (rs_) return true;
    const double c[5] = {K_.fx, K_.fy, K_.cx, K_.cy, K_.baseline};
    for (double v : c)
      if (!std::isfinite(v)) { last_error_ = "RansacVerifier: every camera value must be finite"; return false; }
    if (!(K_.fx > 0) || !(K_.fy > 0) || !(K_.baseline > 0)) { last_error_ = "RansacVerifier: fx, fy and baseline must be > 0"; return false; }
    if (sship_ransac_create(max_obs_, 1, &rs_) != SSHIP_OK) { last_error_ = sship_last_error(); rs_ = nullptr; return false; }
    if (sship_ransac_set_camera(rs_, K_.fx, K_.fy, K_.cx, K_.cy, K_.baseline) != SSHIP_OK || sship_ransac_set_params(rs_, &params_) != SSHIP_OK) {
      last_error_ = sship_last_error();
      sship_ransac_destroy(rs_); rs_ = nullptr;
      return false;
    }
    return true;
  }
  StereoCalibration K_;
  int max_obs_;
  sship_ransac_params params_;
  sship_ransac* rs_ = nullptr;
  std::vector<float> pts_, meas_;
  std::string last_error_;
};

}  // namespace superslam_hip
