// superslam_hip/pose_graph.hpp - the batch pose graph over keyframe poses above the C ABI (include/sship.h "Pose graph"):
// superslam_hip::PoseGraph has the surface of superslam::GlobalPoseGraph (include/GlobalPoseGraph.h): add_keyframe, add_odometry, add_loop,
// optimize_and_get_all, pose_of, size, has, last_loop_rejected.  A pose is a Pose3x4 (trajectory.hpp): Twc, row-major [R | t].  A noise
// model is its six sigmas (rotation x3, translation x3) and, for a loop, the Huber k^2 (<= 0: none).  Before the solve the class does what
// the reference does: a non-finite initial pose or odometry measurement becomes the identity, a non-finite loop is not added, keyframe ids
// map to insertion indices, an odometry edge between keyframes that are not consecutive in insertion order becomes a loop record without a
// robust kernel.  optimize_and_get_all() makes one sship_pg_solve_host call; the estimate becomes the seed of the next solve, and the
// loops that the rejection loop dropped are removed for good (last_loop_rejected() tells that it happened).
// The handle is created by the first optimize_and_get_all().  A failed call returns false / the previous estimate, never throws, and
// records last_error().  Bad arguments (sizes, parameters, unknown ids, a sigma that is not > 0) are refused without touching a device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "../sship.h"
#include "pose_solver.hpp"
#include "trajectory.hpp"

namespace superslam_hip {

struct EdgeNoise {
  double sigma[6] = {0.02, 0.02, 0.02, 0.05, 0.05, 0.05};   // rotation x3, translation x3
  double huber_k2 = 0.0;                                    // loops only; <= 0: no robust kernel
};

class PoseGraph {
public:
  struct Report {
    int n_edges = 0, loops_dropped = 0, trials = 0, status = SSHIP_PG_TOO_FEW;
    double cost_initial = 0.0, cost = 0.0;
  };
  static sship_pg_params default_params() { return sship_pg_params{0.02, 0.05, 1e-5, 1e5, 1e-5, 1e-5, 1e6, 100}; }

  explicit PoseGraph(int max_nodes = 4096, int max_loops = 128) : max_nodes_(max_nodes), max_loops_(max_loops), params_(default_params()) {}
  ~PoseGraph() { if (pg_) sship_pg_destroy(pg_); }
  PoseGraph(const PoseGraph&) = delete;
  PoseGraph& operator=(const PoseGraph&) = delete;

  bool set_params(const sship_pg_params& p) {
    if (!check_params(p)) return false;
    if (pg_ && sship_pg_set_params(pg_, &p) != SSHIP_OK) { last_error_ = sship_last_error(); return false; }
    params_ = p;
    return true;
  }
  const sship_pg_params& params() const { return params_; }

  // a keyframe node with its initial estimate; the first one is the gauge (is_first is kept for the surface: node 0 is held fixed).
  // false: the id is known already, or the graph is full
  bool add_keyframe(size_t keyframe_id, const Pose3x4& initial, bool is_first = false) {
    (void)is_first;
    if (index_.count(keyframe_id)) { last_error_ = "PoseGraph::add_keyframe: the keyframe is in the graph already"; return false; }
    if (ids_.size() >= static_cast<size_t>(max_nodes_ > 0 ? max_nodes_ : 0)) { last_error_ = "PoseGraph::add_keyframe: more keyframes than max_nodes"; return false; }
    index_[keyframe_id] = static_cast<int32_t>(ids_.size());
    ids_.push_back(keyframe_id);
    const Pose3x4 T = finite(initial) ? initial : PoseSolver::identity();
    for (double v : T) pose_.push_back(v);
    if (ids_.size() > 1) {   // the slot towards this node: absent until add_odometry fills it
      odom_z_.insert(odom_z_.end(), 12, std::numeric_limits<double>::quiet_NaN());
      odom_sigma_.insert(odom_sigma_.end(), 6, 1.0);
    }
    return true;
  }

  // rel = T_from^-1 T_to.  Between keyframes consecutive in insertion order it is the backbone's slot; otherwise a loop record without a
  // robust kernel
  bool add_odometry(size_t from, size_t to, const Pose3x4& rel, const EdgeNoise& noise) {
    int32_t i, j;
    if (!edge_args("add_odometry", from, to, noise, &i, &j)) return false;
    const Pose3x4 Z = finite(rel) ? rel : PoseSolver::identity();
    if (j == i + 1) {
      for (int q = 0; q < 12; ++q) odom_z_[static_cast<size_t>(i) * 12 + q] = Z[q];
      for (int q = 0; q < 6; ++q) odom_sigma_[static_cast<size_t>(i) * 6 + q] = noise.sigma[q];
      return true;
    }
    return push_loop("add_odometry", i, j, Z, noise.sigma, 0.0);
  }

  // a loop closure; a non-finite measurement is not added (true: nothing to do, as in the reference)
  bool add_loop(size_t from, size_t to, const Pose3x4& rel, const EdgeNoise& noise) {
    int32_t i, j;
    if (!edge_args("add_loop", from, to, noise, &i, &j)) return false;
    if (!finite(rel)) return true;
    return push_loop("add_loop", i, j, rel, noise.sigma, noise.huber_k2);
  }

  // one solve; the poses of all keyframes by id.  On a failed call the previous estimate comes back and last_error() says why
  std::map<size_t, Pose3x4> optimize_and_get_all() {
    report_ = Report();
    last_loop_rejected_ = false;
    if (solve()) {
      last_loop_rejected_ = report_.loops_dropped > 0;
      for (int d = 0; d < report_.loops_dropped && !loop_k2_.empty(); ++d) {   // the dropped ones are the last present ones: all are present here
        loop_ij_.resize(loop_ij_.size() - 2); loop_z_.resize(loop_z_.size() - 12); loop_sigma_.resize(loop_sigma_.size() - 6); loop_k2_.pop_back();
      }
    }
    std::map<size_t, Pose3x4> all;
    for (size_t k = 0; k < ids_.size(); ++k) all[ids_[k]] = at(k);
    return all;
  }

  // the current estimate; identity for a keyframe that is not in the graph
  Pose3x4 pose_of(size_t keyframe_id) const {
    const auto it = index_.find(keyframe_id);
    return it == index_.end() ? PoseSolver::identity() : at(static_cast<size_t>(it->second));
  }
  size_t size() const { return ids_.size(); }
  bool has(size_t keyframe_id) const { return index_.count(keyframe_id) != 0; }
  bool last_loop_rejected() const { return last_loop_rejected_; }
  size_t loop_count() const { return loop_k2_.size(); }
  const Report& report() const { return report_; }
  const std::string& last_error() const { return last_error_; }
  sship_pg* handle() const { return pg_; }

private:
  static bool finite(const Pose3x4& T) {
    for (double v : T)
      if (!std::isfinite(v)) return false;
    return true;
  }
  Pose3x4 at(size_t k) const {
    Pose3x4 T{};
    for (int q = 0; q < 12; ++q) T[q] = pose_[k * 12 + q];
    return T;
  }
  bool edge_args(const char* who, size_t from, size_t to, const EdgeNoise& noise, int32_t* i, int32_t* j) {
    const auto a = index_.find(from), b = index_.find(to);
    if (a == index_.end() || b == index_.end() || from == to) { last_error_ = std::string("PoseGraph::") + who + ": two different keyframes of the graph are needed"; return false; }
    for (double s : noise.sigma)
      if (!(s > 0) || !std::isfinite(s)) { last_error_ = std::string("PoseGraph::") + who + ": every sigma must be finite and > 0"; return false; }
    if (noise.huber_k2 != noise.huber_k2 || std::isinf(noise.huber_k2)) { last_error_ = std::string("PoseGraph::") + who + ": huber_k2 must be finite"; return false; }
    *i = a->second; *j = b->second;
    return true;
  }
  bool push_loop(const char* who, int32_t i, int32_t j, const Pose3x4& Z, const double* sigma, double k2) {
    if (loop_k2_.size() >= static_cast<size_t>(max_loops_ > 0 ? max_loops_ : 0)) { last_error_ = std::string("PoseGraph::") + who + ": more loops than max_loops"; return false; }
    loop_ij_.push_back(i); loop_ij_.push_back(j);
    for (double v : Z) loop_z_.push_back(v);
    for (int q = 0; q < 6; ++q) loop_sigma_.push_back(sigma[q]);
    loop_k2_.push_back(k2);
    return true;
  }
  bool check_params(const sship_pg_params& p) {
    const double all[7] = {p.odom_sigma_rot, p.odom_sigma_trans, p.lambda0, p.lambda_max, p.abs_tol, p.rel_tol, p.max_translation};
    for (double v : all)
      if (v != v) { last_error_ = "PoseGraph: a parameter is NaN"; return false; }
    if (!(p.odom_sigma_rot > 0) || !(p.odom_sigma_trans > 0) || std::isinf(p.odom_sigma_rot) || std::isinf(p.odom_sigma_trans)) {
      last_error_ = "PoseGraph: odom_sigma_rot and odom_sigma_trans must be finite and > 0"; return false;
    }
    if (!(p.lambda0 > 0) || p.lambda_max < p.lambda0 || std::isinf(p.lambda_max)) { last_error_ = "PoseGraph: lambda0 must be > 0 and lambda_max finite and >= lambda0"; return false; }
    if (p.abs_tol < 0 || p.rel_tol < 0) { last_error_ = "PoseGraph: a tolerance is negative"; return false; }
    if (!(p.max_translation > 0) || std::isinf(p.max_translation)) { last_error_ = "PoseGraph: max_translation must be finite and > 0"; return false; }
    if (p.max_iterations < 1) { last_error_ = "PoseGraph: max_iterations must be >= 1"; return false; }
    return true;
  }
  bool ensure() {
    if (pg_) return true;
    if (max_nodes_ < 2 || max_nodes_ > 4096) { last_error_ = "PoseGraph: max_nodes must be in [2, 4096]"; return false; }
    if (max_loops_ < 0 || max_loops_ > 128) { last_error_ = "PoseGraph: max_loops must be in [0, 128]"; return false; }
    if (sship_pg_create(max_nodes_, max_loops_, 1, &pg_) != SSHIP_OK) { last_error_ = sship_last_error(); pg_ = nullptr; return false; }
    if (sship_pg_set_params(pg_, &params_) != SSHIP_OK) {
      last_error_ = sship_last_error();
      sship_pg_destroy(pg_); pg_ = nullptr;
      return false;
    }
    return true;
  }
  bool solve() {
    if (!ensure()) return false;
    out_.assign(pose_.size(), 0.0);
    int32_t stats[4] = {0, 0, 0, 0};
    double cost[2] = {0.0, 0.0};
    if (sship_pg_solve_host(pg_, static_cast<int>(ids_.size()), pose_.data(), odom_z_.data(), odom_sigma_.data(), static_cast<int>(loop_k2_.size()),
                            loop_ij_.data(), loop_z_.data(), loop_sigma_.data(), loop_k2_.data(), out_.data(), stats, cost, nullptr) != SSHIP_OK) {
      last_error_ = sship_last_error();
      return false;
    }
    report_.n_edges = stats[0]; report_.loops_dropped = stats[1]; report_.trials = stats[2]; report_.status = stats[3];
    report_.cost_initial = cost[0]; report_.cost = cost[1];
    pose_ = out_;   // the estimate is the next seed (TOO_FEW, BAD_INPUT and DIVERGED hand the seed back)
    return true;
  }
  int max_nodes_, max_loops_;
  sship_pg_params params_;
  sship_pg* pg_ = nullptr;
  std::vector<size_t> ids_;                   // keyframe ids in insertion order
  std::map<size_t, int32_t> index_;           // id -> insertion index
  std::vector<double> pose_, out_;            // the current estimate [n, 12]
  std::vector<double> odom_z_, odom_sigma_;   // [n - 1, 12], [n - 1, 6]; a slot that add_odometry has not filled is NaN, hence absent
  std::vector<int32_t> loop_ij_;
  std::vector<double> loop_z_, loop_sigma_, loop_k2_;
  bool last_loop_rejected_ = false;
  std::string last_error_;
  Report report_;
};

}  // namespace superslam_hip
