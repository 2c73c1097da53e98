// superslam_hip/window_smoother.hpp - the fixed-lag window of keyframe poses above the C ABI (include/sship.h "Window smoother"):
// superslam_hip::WindowSmoother has the surface of superslam::WindowSmoother (include/WindowSmoother.h): add_keyframe with the fixed-lag
// drop of the oldest, optimize, pose_of, window_count, in_window.  An observation is the reference's StereoObs {landmark_id, meas} as plain
// values; the solver reads fp32, so the measurements are narrowed once on the way in.  A pose is a Pose3x4 (trajectory.hpp): Twc, row-major
// [R | t].  optimize() numbers the window's landmark ids by first appearance (slot after slot, row after row), makes one
// sship_ba_solve_host call and keeps the previous poses unless the status is CONVERGED or ITER_CAP - the reference's "keep on failure"
// (src/WindowSmoother.cc:103-116).  The objective is the reference's, the schedule the library's own (stated in sship.h).
// The handle is created by the first optimize().  A failed call returns false, never throws, and records last_error().  Bad arguments
// (camera, parameters, sizes, more observations in a keyframe than max_obs) are refused without touching a device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "../sship.h"
#include "pose_solver.hpp"
#include "trajectory.hpp"

namespace superslam_hip {

struct StereoObs {
  size_t landmark_id = 0;
  double uL = 0.0, uR = 0.0, v = 0.0;
};

class WindowSmoother {
public:
  struct Report {
    int n_obs = 0, n_landmarks = 0, trials = 0, status = SSHIP_BA_TOO_FEW;
    double cost_initial = 0.0, cost = 0.0;
  };
  static sship_ba_params default_params() { return sship_ba_params{1.0, 9.0, 1e-5, 1e5, 1e-3, 1e-3, 20}; }

  WindowSmoother(const StereoCalibration& K, size_t window_size, int max_obs = 600)
      : K_(K), window_size_(window_size), max_obs_(max_obs), params_(default_params()) {}
  ~WindowSmoother() { if (ba_) sship_ba_destroy(ba_); }
  WindowSmoother(const WindowSmoother&) = delete;
  WindowSmoother& operator=(const WindowSmoother&) = delete;

  bool set_params(const sship_ba_params& p) {
    if (!check_params(p)) return false;
    if (ba_ && sship_ba_set_params(ba_, &p) != SSHIP_OK) { last_error_ = sship_last_error(); return false; }
    params_ = p;
    return true;
  }
  const sship_ba_params& params() const { return params_; }

  // the newest keyframe; past window_size the oldest leaves with its pose and observations.  false: more observations than max_obs
  bool add_keyframe(size_t keyframe_id, const Pose3x4& initial_pose, const std::vector<StereoObs>& obs) {
    if (obs.size() > static_cast<size_t>(max_obs_ > 0 ? max_obs_ : 0)) { last_error_ = "WindowSmoother::add_keyframe: more observations than max_obs"; return false; }
    window_.push_back(keyframe_id);
    poses_[keyframe_id] = initial_pose;
    obs_by_kf_[keyframe_id] = obs;
    while (window_.size() > window_size_ && !window_.empty()) {
      const size_t old = window_.front();
      window_.pop_front();
      poses_.erase(old);
      obs_by_kf_.erase(old);
    }
    return true;
  }

  // one solve over the window.  true: the call ran (report() tells how it ended); the poses are replaced on CONVERGED and ITER_CAP only
  bool optimize() {
    report_ = Report();
    if (!ensure()) return false;
    const size_t K = window_size_, N = static_cast<size_t>(max_obs_);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    meas_.assign(K * N * 3, nan);
    track_.assign(K * N, -1);
    pose0_.assign(K * 12, 0.0);
    std::map<size_t, int32_t> number;                                   // landmark id -> its number, by first appearance
    for (size_t k = 0; k < window_.size(); ++k) {
      const Pose3x4& T = poses_[window_[k]];
      for (int i = 0; i < 12; ++i) pose0_[k * 12 + i] = T[i];
      const std::vector<StereoObs>& obs = obs_by_kf_[window_[k]];
      for (size_t i = 0; i < obs.size(); ++i) {
        auto it = number.find(obs[i].landmark_id);
        if (it == number.end()) it = number.emplace(obs[i].landmark_id, static_cast<int32_t>(number.size())).first;
        track_[k * N + i] = it->second;
        meas_[(k * N + i) * 3] = static_cast<float>(obs[i].uL);
        meas_[(k * N + i) * 3 + 1] = static_cast<float>(obs[i].uR);
        meas_[(k * N + i) * 3 + 2] = static_cast<float>(obs[i].v);
      }
    }
    out_.assign(K * 12, 0.0);
    int32_t stats[4] = {0, 0, 0, 0};
    double cost[2] = {0.0, 0.0};
    if (sship_ba_solve_host(ba_, meas_.data(), track_.data(), static_cast<int>(window_.size()), pose0_.data(), out_.data(), stats, cost, nullptr) !=
        SSHIP_OK) {
      last_error_ = sship_last_error();
      return false;
    }
    report_.n_obs = stats[0]; report_.n_landmarks = stats[1]; report_.trials = stats[2]; report_.status = stats[3];
    report_.cost_initial = cost[0]; report_.cost = cost[1];
    if (stats[3] == SSHIP_BA_CONVERGED || stats[3] == SSHIP_BA_ITER_CAP)
      for (size_t k = 0; k < window_.size(); ++k) {
        Pose3x4& T = poses_[window_[k]];
        for (int i = 0; i < 12; ++i) T[i] = out_[k * 12 + i];
      }
    return true;
  }

  // the current estimate; identity for a keyframe that is not in the window
  Pose3x4 pose_of(size_t keyframe_id) const {
    const auto it = poses_.find(keyframe_id);
    return it == poses_.end() ? PoseSolver::identity() : it->second;
  }
  size_t window_count() const { return window_.size(); }
  bool in_window(size_t keyframe_id) const { return poses_.count(keyframe_id) != 0; }
  const Report& report() const { return report_; }
  int max_obs() const { return max_obs_; }
  const std::string& last_error() const { return last_error_; }
  sship_ba* handle() const { return ba_; }

private:
  bool check_params(const sship_ba_params& p) {
    const double all[6] = {p.sigma_px, p.huber_k2, p.lambda0, p.lambda_max, p.abs_tol, p.rel_tol};
    for (double v : all)
      if (v != v) { last_error_ = "WindowSmoother: a parameter is NaN"; return false; }
    if (!(p.sigma_px > 0) || !(p.huber_k2 > 0) || std::isinf(p.sigma_px) || std::isinf(p.huber_k2)) {
      last_error_ = "WindowSmoother: sigma_px and huber_k2 must be finite and > 0"; return false;
    }
    if (!(p.lambda0 > 0) || p.lambda_max < p.lambda0 || std::isinf(p.lambda_max)) { last_error_ = "WindowSmoother: lambda0 must be > 0 and lambda_max finite and >= lambda0"; return false; }
    if (p.abs_tol < 0 || p.rel_tol < 0) { last_error_ = "WindowSmoother: a tolerance is negative"; return false; }
    if (p.max_iterations < 1) { last_error_ = "WindowSmoother: max_iterations must be >= 1"; return false; }
    return true;
  }
  bool ensure() {
    if (ba_) return true;
    const double c[5] = {K_.fx, K_.fy, K_.cx, K_.cy, K_.baseline};
    for (double v : c)
      if (!std::isfinite(v)) { last_error_ = "WindowSmoother: every camera value must be finite"; return false; }
    if (!(K_.fx > 0) || !(K_.fy > 0) || !(K_.baseline > 0)) { last_error_ = "WindowSmoother: fx, fy and baseline must be > 0"; return false; }
    if (window_size_ < 2 || window_size_ > 16) { last_error_ = "WindowSmoother: window_size must be in [2, 16]"; return false; }
    if (max_obs_ < 1 || max_obs_ > 2048) { last_error_ = "WindowSmoother: max_obs must be in [1, 2048]"; return false; }
    const int K = static_cast<int>(window_size_);
    if (sship_ba_create(K, max_obs_, K * max_obs_, 1, &ba_) != SSHIP_OK) { last_error_ = sship_last_error(); ba_ = nullptr; return false; }
    if (sship_ba_set_camera(ba_, K_.fx, K_.fy, K_.cx, K_.cy, K_.baseline) != SSHIP_OK || sship_ba_set_params(ba_, &params_) != SSHIP_OK) {
      last_error_ = sship_last_error();
      sship_ba_destroy(ba_); ba_ = nullptr;
      return false;
    }
    return true;
  }
  StereoCalibration K_;
  size_t window_size_;
  int max_obs_;
  sship_ba_params params_;
  sship_ba* ba_ = nullptr;
  std::deque<size_t> window_;                            // keyframe ids in window order, the oldest first
  std::map<size_t, Pose3x4> poses_;                      // the current estimate per keyframe id
  std::map<size_t, std::vector<StereoObs>> obs_by_kf_;   // observations per keyframe id
  std::vector<float> meas_;
  std::vector<int32_t> track_;
  std::vector<double> pose0_, out_;
  std::string last_error_;
  Report report_;
};

}  // namespace superslam_hip
