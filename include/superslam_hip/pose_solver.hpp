// superslam_hip/pose_solver.hpp - the pose-only stereo solve above the C ABI (include/sship.h "Pose-only stereo solver"):
// superslam_hip::PoseSolver::track(initial, observations) takes the place of one superslam::FrameTracker::track call (src/FrameTracker.cc)
// and of LoopCloser::verify's solve plus its inlier count (src/LoopCloser.cc:55-89).  An observation is the reference's PointObs {Xw, meas}
// as plain doubles; the solver reads fp32, so the values are narrowed once on the way in.  A pose is a Pose3x4 (trajectory.hpp): Twc,
// row-major [R | t].  The objective is FrameTracker's; the Levenberg-Marquardt schedule is the library's own (stated in sship.h).
// The handle is created by the first solve.  A failed call returns ok = false with the pose it was given, never throws, and records
// last_error().  Bad arguments (camera, parameters, more observations than max_obs) are refused without touching a device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../sship.h"
#include "trajectory.hpp"

namespace superslam_hip {

struct StereoCalibration {
  double fx, fy, cx, cy, baseline;
};

struct StereoPointObs {
  double X, Y, Z;      // the landmark in the frame the pose maps into (PointObs::Xw)
  double uL, uR, v;    // its stereo measurement in the frame being solved (PointObs::meas)
};

class PoseSolver {
public:
  struct Result {
    bool ok = false;
    Pose3x4 pose{};
    int n_obs = 0, n_inliers = 0, trials = 0, status = SSHIP_POSE_BAD_INPUT;
    double cost_initial = 0.0, cost = 0.0;
  };
  static Pose3x4 identity() { return Pose3x4{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}; }
  static sship_pose_params default_params() { return sship_pose_params{10.0, 8.0, 40.0, 7.815, 1e-5, 1e5, 1e-5, 1e-5, 3.0, 100}; }

  explicit PoseSolver(const StereoCalibration& K, int max_obs = 2048) : K_(K), max_obs_(max_obs), params_(default_params()) {}
  ~PoseSolver() { if (ps_) sship_pose_destroy(ps_); }
  PoseSolver(const PoseSolver&) = delete;
  PoseSolver& operator=(const PoseSolver&) = delete;

  // the rule's constants; false (last_error()) and the old values kept for a NaN, a non-positive sigma, a negative tolerance, ...
  bool set_params(const sship_pose_params& p) {
    if (!check_params(p)) return false;
    if (ps_ && sship_pose_set_params(ps_, &p) != SSHIP_OK) { last_error_ = sship_last_error(); return false; }
    params_ = p;
    return true;
  }
  const sship_pose_params& params() const { return params_; }

  // FrameTracker::track.  inliers (optional) receives one byte per observation: the reprojection inliers at the pose returned.
  Result track(const Pose3x4& initial_guess, const std::vector<StereoPointObs>& matches, std::vector<uint8_t>* inliers = nullptr) {
    Result r;
    r.pose = initial_guess;
    const size_t n = matches.size();
    if (n > static_cast<size_t>(max_obs_ > 0 ? max_obs_ : 0)) { last_error_ = "PoseSolver::track: more observations than max_obs"; return r; }
    if (!ensure()) return r;
    pts_.resize(3 * n); meas_.resize(3 * n);
    for (size_t i = 0; i < n; ++i) {
      const StereoPointObs& o = matches[i];
      pts_[3 * i] = static_cast<float>(o.X); pts_[3 * i + 1] = static_cast<float>(o.Y); pts_[3 * i + 2] = static_cast<float>(o.Z);
      meas_[3 * i] = static_cast<float>(o.uL); meas_[3 * i + 1] = static_cast<float>(o.uR); meas_[3 * i + 2] = static_cast<float>(o.v);
    }
    if (inliers) inliers->assign(n, 0);
    int32_t stats[4] = {0, 0, 0, 0};
    double cost[2] = {0.0, 0.0};
    Pose3x4 out{};
    if (sship_pose_solve_host(ps_, pts_.data(), meas_.data(), nullptr, static_cast<int>(n), initial_guess.data(), out.data(), stats, cost,
                              inliers && n ? inliers->data() : nullptr) != SSHIP_OK) {
      last_error_ = sship_last_error();
      return r;
    }
    r.ok = true; r.pose = out;
    r.n_obs = stats[0]; r.n_inliers = stats[1]; r.trials = stats[2]; r.status = stats[3];
    r.cost_initial = cost[0]; r.cost = cost[1];
    return r;
  }
  // LoopCloser::verify's solve: seeded at identity
  Result track(const std::vector<StereoPointObs>& matches, std::vector<uint8_t>* inliers = nullptr) { return track(identity(), matches, inliers); }

  // LoopCloser.cc:19-24: the stereo point (uL, uR, v) in the camera frame
  StereoPointObs backproject(double uL, double uR, double v) const {
    const double Z = K_.fx * K_.baseline / (uL - uR);
    return StereoPointObs{(uL - K_.cx) * Z / K_.fx, (v - K_.cy) * Z / K_.fy, Z, 0.0, 0.0, 0.0};
  }
  int max_obs() const { return max_obs_; }
  const StereoCalibration& calibration() const { return K_; }
  const std::string& last_error() const { return last_error_; }
  sship_pose* handle() const { return ps_; }

private:
  bool check_params(const sship_pose_params& p) {
    const double all[9] = {p.sigma_px, p.sigma_d0, p.cond_depth, p.huber_k2, p.lambda0, p.lambda_max, p.abs_tol, p.rel_tol, p.inlier_px};
    for (double v : all)
      if (v != v) { last_error_ = "PoseSolver: a parameter is NaN"; return false; }
    if (!(p.sigma_px > 0) || !(p.sigma_d0 > 0) || !(p.cond_depth > 0) || !(p.huber_k2 > 0) || std::isinf(p.sigma_px) || std::isinf(p.sigma_d0) ||
        std::isinf(p.cond_depth) || std::isinf(p.huber_k2)) {
      last_error_ = "PoseSolver: sigma_px, sigma_d0, cond_depth and huber_k2 must be finite and > 0"; return false;
    }
    if (!(p.lambda0 > 0) || p.lambda_max < p.lambda0 || std::isinf(p.lambda_max)) { last_error_ = "PoseSolver: lambda0 must be > 0 and lambda_max finite and >= lambda0"; return false; }
    if (p.abs_tol < 0 || p.rel_tol < 0 || p.inlier_px < 0) { last_error_ = "PoseSolver: a tolerance or inlier_px is negative"; return false; }
    if (p.max_iterations < 1) { last_error_ = "PoseSolver: max_iterations must be >= 1"; return false; }
    return true;
  }
  bool ensure() {
    if (ps_) return true;
    const double c[5] = {K_.fx, K_.fy, K_.cx, K_.cy, K_.baseline};
    for (double v : c)
      if (!std::isfinite(v)) { last_error_ = "PoseSolver: every camera value must be finite"; return false; }
    if (!(K_.fx > 0) || !(K_.fy > 0) || !(K_.baseline > 0)) { last_error_ = "PoseSolver: fx, fy and baseline must be > 0"; return false; }
    if (sship_pose_create(max_obs_, 1, &ps_) != SSHIP_OK) { last_error_ = sship_last_error(); ps_ = nullptr; return false; }
    if (sship_pose_set_camera(ps_, K_.fx, K_.fy, K_.cx, K_.cy, K_.baseline) != SSHIP_OK || sship_pose_set_params(ps_, &params_) != SSHIP_OK) {
      last_error_ = sship_last_error();
      sship_pose_destroy(ps_); ps_ = nullptr;
      return false;
    }
    return true;
  }
  StereoCalibration K_;
  int max_obs_;
  sship_pose_params params_;
  sship_pose* ps_ = nullptr;
  std::vector<float> pts_, meas_;
  std::string last_error_;
};

}  // namespace superslam_hip
