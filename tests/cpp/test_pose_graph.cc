// The C++ host layer's pose graph (include/superslam_hip/pose_graph.hpp: superslam_hip::PoseGraph).
//   no arguments : CPU - the graph's bookkeeping (ids, has, size, pose_of, the identity substitutions), the class's argument validation
//                  (false, last_error, nothing thrown) and the C ABI's argument checks (refused before any device is touched)
//   gpu          : GPU - the reference's two unit tests (tests/test_global_pose_graph.cc: the four-node chain recovered to 1e-3, the
//                  octagon's drift more than halved by the loop) through the class, last_loop_rejected with an absurd loop, the estimate
//                  as the next seed, and the refusals on a live handle
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#include "superslam_hip/pose_graph.hpp"

using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static Pose3x4 rz(double a, double x, double y, double z) { return Pose3x4{std::cos(a), -std::sin(a), 0, x, std::sin(a), std::cos(a), 0, y, 0, 0, 1, z}; }
static Pose3x4 mul(const Pose3x4& A, const Pose3x4& B) {
  Pose3x4 C{};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) C[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j];
    C[4 * i + 3] = A[4 * i] * B[3] + A[4 * i + 1] * B[7] + A[4 * i + 2] * B[11] + A[4 * i + 3];
  }
  return C;
}
static Pose3x4 between(const Pose3x4& A, const Pose3x4& B) {
  Pose3x4 C{};
  const double d[3] = {B[3] - A[3], B[7] - A[7], B[11] - A[11]};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) C[4 * i + j] = A[i] * B[j] + A[4 + i] * B[4 + j] + A[8 + i] * B[8 + j];
    C[4 * i + 3] = A[i] * d[0] + A[4 + i] * d[1] + A[8 + i] * d[2];
  }
  return C;
}
static double distance(const Pose3x4& A, const Pose3x4& B) { return std::sqrt((A[3] - B[3]) * (A[3] - B[3]) + (A[7] - B[7]) * (A[7] - B[7]) + (A[11] - B[11]) * (A[11] - B[11])); }
static double max_diff(const Pose3x4& A, const Pose3x4& B) {
  double m = 0.0;
  for (int i = 0; i < 12; ++i) m = std::fmax(m, std::fabs(A[i] - B[i]));
  return m;
}
static EdgeNoise odom_noise() {
  EdgeNoise n;
  for (int i = 0; i < 6; ++i) n.sigma[i] = i < 3 ? 0.05 : 0.1;
  return n;
}

static int run_cpu() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const Pose3x4 I = PoseSolver::identity();
  {
    PoseGraph g(8, 2);
    EXPECT(g.size() == 0 && !g.has(3) && g.pose_of(3) == I && g.handle() == nullptr && !g.last_loop_rejected());
    EXPECT(g.add_keyframe(10, rz(0.1, 1, 2, 3), true) && g.add_keyframe(7, rz(0.2, 2, 2, 3), false) && g.add_keyframe(42, rz(0.3, 3, 2, 3), false));
    EXPECT(g.size() == 3 && g.has(7) && !g.has(8) && g.pose_of(42) == rz(0.3, 3, 2, 3));
    EXPECT(!g.add_keyframe(7, I, false) && g.last_error().find("already") != std::string::npos && g.size() == 3);
    Pose3x4 bad = I;
    bad[5] = nan;
    EXPECT(g.add_keyframe(5, bad, false) && g.pose_of(5) == I);                                 // a non-finite initial pose becomes the identity
    EXPECT(g.add_odometry(10, 7, bad, odom_noise()));                                           // and so does a non-finite odometry measurement
    EXPECT(g.add_odometry(10, 42, I, odom_noise()) && g.loop_count() == 1);                     // not consecutive: a loop record
    EXPECT(g.add_loop(5, 10, bad, odom_noise()) && g.loop_count() == 1);                        // a non-finite loop is not added
    EXPECT(g.add_loop(5, 10, I, odom_noise()) && g.loop_count() == 2);
    EXPECT(!g.add_loop(42, 10, I, odom_noise()) && g.last_error().find("max_loops") != std::string::npos);
    EXPECT(!g.add_loop(42, 99, I, odom_noise()) && !g.add_loop(42, 42, I, odom_noise()) && !g.add_odometry(99, 42, I, odom_noise()));
    EdgeNoise zero = odom_noise();
    zero.sigma[4] = 0.0;
    EXPECT(!g.add_odometry(7, 42, I, zero) && g.last_error().find("sigma") != std::string::npos);
    for (size_t id = 100; id < 104; ++id) EXPECT(g.add_keyframe(id, I, false));
    EXPECT(!g.add_keyframe(200, I, false) && g.last_error().find("max_nodes") != std::string::npos && g.size() == 8);
    sship_pg_params p = PoseGraph::default_params();
    EXPECT(p.odom_sigma_rot == 0.02 && p.odom_sigma_trans == 0.05 && p.lambda0 == 1e-5 && p.lambda_max == 1e5 && p.abs_tol == 1e-5 && p.rel_tol == 1e-5 &&
           p.max_translation == 1e6 && p.max_iterations == 100);
    EXPECT(g.set_params(p));
    p.max_iterations = 0; EXPECT(!g.set_params(p) && g.params().max_iterations == 100);
    p = PoseGraph::default_params(); p.abs_tol = -1.0; EXPECT(!g.set_params(p));
    p = PoseGraph::default_params(); p.rel_tol = nan; EXPECT(!g.set_params(p) && g.last_error().find("NaN") != std::string::npos);
    p = PoseGraph::default_params(); p.odom_sigma_trans = 0.0; EXPECT(!g.set_params(p));
    p = PoseGraph::default_params(); p.lambda0 = 0.0; EXPECT(!g.set_params(p));
    p = PoseGraph::default_params(); p.lambda_max = 1e-9; EXPECT(!g.set_params(p));
    p = PoseGraph::default_params(); p.max_translation = std::numeric_limits<double>::infinity(); EXPECT(!g.set_params(p));
  }
  {
    PoseGraph small(1, 0), wide(4097, 0), loops(8, 129);
    EXPECT(small.optimize_and_get_all().empty() && small.last_error().find("max_nodes") != std::string::npos && small.handle() == nullptr);
    EXPECT(wide.optimize_and_get_all().empty() && wide.last_error().find("max_nodes") != std::string::npos);
    EXPECT(loops.optimize_and_get_all().empty() && loops.last_error().find("max_loops") != std::string::npos);
  }
  sship_pg* out = nullptr;
  EXPECT(sship_pg_create(1, 0, 1, &out) == SSHIP_ERR_INVALID && out == nullptr && sship_pg_create(4097, 0, 1, &out) == SSHIP_ERR_INVALID);
  EXPECT(sship_pg_create(8, -1, 1, &out) == SSHIP_ERR_INVALID && sship_pg_create(8, 129, 1, &out) == SSHIP_ERR_INVALID);
  EXPECT(sship_pg_create(8, 4, 0, &out) == SSHIP_ERR_INVALID && sship_pg_create(8, 4, 65536, &out) == SSHIP_ERR_INVALID);
  EXPECT(sship_pg_create(8, 4, 1, nullptr) == SSHIP_ERR_INVALID);
  sship_pg_params p = PoseGraph::default_params();
  double d = 0.0; float f = 0.f; int32_t st[4]; uint8_t u = 0;
  EXPECT(sship_pg_set_params(nullptr, &p) == SSHIP_ERR_INVALID && sship_pg_get_params(nullptr, &p) == SSHIP_ERR_INVALID);
  EXPECT(sship_pg_solve_batch_device(nullptr, nullptr, &d, &d, nullptr, st, &d, &d, &d, nullptr, 1, &d, st, &d, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_pg_solve_host(nullptr, 2, &d, &d, nullptr, 0, nullptr, nullptr, nullptr, nullptr, &d, st, &d, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_pg_odometry_from_poses_batch_device(nullptr, &d, 1, &d, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_pg_loops_from_pose_batch_device(nullptr, st, st, &d, st, 1, 30, 0.1, st, &d, &d, &d, &u, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_pg_bench(nullptr, 1, &f) == SSHIP_ERR_INVALID);
  sship_pg_destroy(nullptr);
  std::printf(g_fail ? "pose graph host layer: %d check(s) failed (cpu)\n" : "pose graph host layer: all checks passed (cpu)\n", g_fail);
  return g_fail ? 1 : 0;
}

static int run_gpu() {
  {  // an exact odometry chain, the seeds perturbed: the truth comes back
    std::vector<Pose3x4> gt = {rz(0, 0, 0, 0), rz(0, 1, 0, 0), rz(0, 2, 0, 0), rz(0, 3, 0, 0)};
    PoseGraph g(16, 4);
    EXPECT(g.add_keyframe(0, gt[0], true));
    for (size_t k = 1; k < gt.size(); ++k) {
      EXPECT(g.add_keyframe(k, mul(gt[k], rz(0.05, 0.2, -0.1, 0.0)), false));
      EXPECT(g.add_odometry(k - 1, k, between(gt[k - 1], gt[k]), odom_noise()));
    }
    std::map<size_t, Pose3x4> poses = g.optimize_and_get_all();
    EXPECT(g.handle() != nullptr && g.report().status == SSHIP_PG_CONVERGED && g.report().n_edges == 3 && poses.size() == 4);
    for (size_t k = 0; k < gt.size(); ++k) EXPECT(max_diff(poses[k], gt[k]) < 1e-3);
    EXPECT(poses[0] == gt[0]);                                                          // the gauge keeps its bits
    sship_pg_params p = PoseGraph::default_params();
    p.max_iterations = 0;
    EXPECT(!g.set_params(p) && g.params().max_iterations == 100);                       // refused on a live handle too, the old values kept
    sship_pg_params got = p;
    EXPECT(sship_pg_set_params(g.handle(), &p) == SSHIP_ERR_INVALID && sship_pg_get_params(g.handle(), &got) == SSHIP_OK && got.max_iterations == 100);
  }
  {  // the octagon with a yaw bias: the loop more than halves the drift
    const int N = 8;
    const double kPi = 3.14159265358979323846;
    std::vector<Pose3x4> gt;
    Pose3x4 p = PoseSolver::identity();
    for (int i = 0; i < N; ++i) { gt.push_back(p); p = mul(p, rz(2 * kPi / N, 1, 0, 0)); }
    const Pose3x4 bias = rz(0.04, 0, 0, 0);
    PoseGraph g(16, 4);
    EXPECT(g.add_keyframe(0, gt[0], true));
    Pose3x4 dead = gt[0];
    for (int k = 1; k < N; ++k) {
      const Pose3x4 odo = mul(between(gt[k - 1], gt[k]), bias);
      dead = mul(dead, odo);
      EXPECT(g.add_keyframe(k, dead, false));
      EXPECT(g.add_odometry(k - 1, k, odo, odom_noise()));
    }
    std::map<size_t, Pose3x4> before = g.optimize_and_get_all();
    const double drift_before = distance(before[N - 1], gt[N - 1]);
    EXPECT(drift_before > 0.05);
    EXPECT(g.add_loop(N - 1, 0, between(gt[N - 1], gt[0]), odom_noise()));
    std::map<size_t, Pose3x4> after = g.optimize_and_get_all();
    const double drift_after = distance(after[N - 1], gt[N - 1]);
    EXPECT(drift_after < 0.5 * drift_before && !g.last_loop_rejected() && g.report().n_edges == N);
    std::printf("octagon: drift %.3f m -> %.3f m in %d trials\n", drift_before, drift_after, g.report().trials);
    // an absurd loop from the gauge with tight sigmas and no robust kernel: dropped by the rejection loop, for good, and the estimate stays
    EdgeNoise tight;
    for (double& s : tight.sigma) s = 1e-3;
    EXPECT(g.add_loop(0, 6, rz(0, 1e9, 0, 0), tight) && g.loop_count() == 2);
    std::map<size_t, Pose3x4> kept = g.optimize_and_get_all();
    EXPECT(g.last_loop_rejected() && g.report().loops_dropped == 1 && g.loop_count() == 1 && g.report().status == SSHIP_PG_CONVERGED);
    EXPECT(distance(kept[N - 1], gt[N - 1]) < 0.5 * drift_before && max_diff(kept[N - 1], after[N - 1]) < 1e-3);
    (void)g.optimize_and_get_all();
    EXPECT(!g.last_loop_rejected() && g.report().trials <= 2);                          // the estimate was the seed: nothing left to do
  }
  std::printf(g_fail ? "pose graph host layer: %d check(s) failed (gpu)\n" : "pose graph host layer: all checks passed (gpu)\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) { return argc > 1 && std::strcmp(argv[1], "gpu") == 0 ? run_gpu() : run_cpu(); }
