// The C++ host layer's pose-only stereo solver (include/superslam_hip/pose_solver.hpp: superslam_hip::PoseSolver).
//   no arguments : CPU - the class's argument validation (ok = false, the pose given back, last_error, nothing thrown) and the C ABI's
//                  argument checks (refused before any device is touched)
//   <in.bin> <out.bin> : GPU - one pair through PoseSolver::track
//       in.bin  = int32 n | f64 camera [5] | f64 pose0 [12] | points f32 [n][3] | meas f32 [n][3]
//       out.bin = f64 pose [12] | int32 stats [4] | f64 cost [2] | u8 inlier [n]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "superslam_hip/pose_solver.hpp"

using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static int run_cpu() {
  const StereoCalibration K{718.856, 718.856, 607.19, 185.22, 0.537};
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<StereoPointObs> obs(4, StereoPointObs{1.0, 0.5, 10.0, 600.0, 560.0, 200.0});
  {
    PoseSolver ps(K, 3);
    EXPECT(ps.max_obs() == 3 && ps.last_error().empty() && ps.handle() == nullptr);
    const PoseSolver::Result r = ps.track(obs);                                       // more observations than max_obs
    EXPECT(!r.ok && r.pose == PoseSolver::identity() && ps.last_error().find("max_obs") != std::string::npos && ps.handle() == nullptr);
    sship_pose_params p = PoseSolver::default_params();
    EXPECT(p.sigma_px == 10.0 && p.sigma_d0 == 8.0 && p.cond_depth == 40.0 && p.huber_k2 == 7.815 && p.inlier_px == 3.0 && p.max_iterations == 100);
    EXPECT(ps.set_params(p));
    p.max_iterations = 0; EXPECT(!ps.set_params(p) && ps.params().max_iterations == 100);
    p = PoseSolver::default_params(); p.abs_tol = -1.0; EXPECT(!ps.set_params(p));
    p = PoseSolver::default_params(); p.rel_tol = nan; EXPECT(!ps.set_params(p) && ps.last_error().find("NaN") != std::string::npos);
    p = PoseSolver::default_params(); p.sigma_px = 0.0; EXPECT(!ps.set_params(p));
    p = PoseSolver::default_params(); p.lambda_max = 1e-9; EXPECT(!ps.set_params(p));
    const StereoPointObs b = ps.backproject(650.0, 610.0, 200.0);
    EXPECT(std::fabs(b.Z - K.fx * K.baseline / 40.0) < 1e-12 && std::fabs(b.X - (650.0 - K.cx) * b.Z / K.fx) < 1e-12);
  }
  for (int which = 0; which < 4; ++which) {                                           // a bad camera: refused without a device
    StereoCalibration bad = K;
    if (which == 0) bad.fx = 0.0;
    if (which == 1) bad.fy = -1.0;
    if (which == 2) bad.baseline = 0.0;
    if (which == 3) bad.cx = nan;
    PoseSolver ps(bad);
    const PoseSolver::Result r = ps.track(obs);
    EXPECT(!r.ok && ps.handle() == nullptr && !ps.last_error().empty());
  }
  {
    PoseSolver none(K, 0), wide(K, 2049);
    EXPECT(!none.track(std::vector<StereoPointObs>()).ok && none.last_error().find("max_obs") != std::string::npos);
    EXPECT(!wide.track(obs).ok && wide.last_error().find("max_obs") != std::string::npos);
  }
  sship_pose* out = nullptr;
  EXPECT(sship_pose_create(0, 1, &out) == SSHIP_ERR_INVALID && out == nullptr);
  EXPECT(sship_pose_create(2049, 1, &out) == SSHIP_ERR_INVALID && sship_pose_create(16, 0, &out) == SSHIP_ERR_INVALID);
  EXPECT(sship_pose_create(16, 65536, &out) == SSHIP_ERR_INVALID && sship_pose_create(16, 1, nullptr) == SSHIP_ERR_INVALID);
  sship_pose_params p = PoseSolver::default_params();
  double d = 0.0; float f = 0.f; int32_t st[4]; uint8_t u = 0; int n = 0;
  EXPECT(sship_pose_set_camera(nullptr, 1, 1, 0, 0, 1) == SSHIP_ERR_INVALID && sship_pose_get_camera(nullptr, &d, &d, &d, &d, &d) == SSHIP_ERR_INVALID);
  EXPECT(sship_pose_set_params(nullptr, &p) == SSHIP_ERR_INVALID && sship_pose_get_params(nullptr, &p) == SSHIP_ERR_INVALID);
  EXPECT(sship_pose_solve_batch_device(nullptr, &f, &f, &u, nullptr, 1, &d, st, &d, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_pose_solve_host(nullptr, &f, &f, &u, 1, nullptr, &d, st, &d, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_pose_obs_from_matches_batch_device(nullptr, &f, &u, &f, &u, st, &n, &n, 1, 1, &f, &f, &u, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_pose_bench(nullptr, 1, &f) == SSHIP_ERR_INVALID);
  sship_pose_destroy(nullptr);
  std::printf(g_fail ? "pose solver host layer: %d check(s) failed (cpu)\n" : "pose solver host layer: all checks passed (cpu)\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return run_cpu();
  std::FILE* fi = std::fopen(argv[1], "rb");
  if (!fi) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int32_t n = 0;
  double cam[5];
  Pose3x4 pose0{};
  if (std::fread(&n, 4, 1, fi) != 1 || n < 0 || n > 2048 || std::fread(cam, 8, 5, fi) != 5 || std::fread(pose0.data(), 8, 12, fi) != 12) return 2;
  std::vector<float> pts(static_cast<size_t>(n) * 3), ms(static_cast<size_t>(n) * 3);
  if (std::fread(pts.data(), 4, pts.size(), fi) != pts.size() || std::fread(ms.data(), 4, ms.size(), fi) != ms.size()) return 2;
  std::fclose(fi);
  std::vector<StereoPointObs> obs(static_cast<size_t>(n));
  for (size_t i = 0; i < obs.size(); ++i) obs[i] = StereoPointObs{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], ms[3 * i], ms[3 * i + 1], ms[3 * i + 2]};
  PoseSolver ps(StereoCalibration{cam[0], cam[1], cam[2], cam[3], cam[4]}, n > 0 ? n : 1);
  std::vector<uint8_t> inl;
  const PoseSolver::Result r = ps.track(pose0, obs, &inl);
  EXPECT(r.ok);
  if (!r.ok) { std::printf("%s\n", ps.last_error().c_str()); return 1; }
  EXPECT(ps.handle() != nullptr && inl.size() == obs.size());
  sship_pose_params p = PoseSolver::default_params();
  p.max_iterations = 0;
  EXPECT(!ps.set_params(p) && ps.params().max_iterations == 100);                     // the class refuses on a live handle too, the old values kept
  // and so does the library underneath the class, for everything the class refuses: called directly on the live handle
  {
    sship_pose* h = ps.handle();
    const sship_pose_params good = PoseSolver::default_params();
    sship_pose_params got = good, bad = good;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    bad = good; bad.max_iterations = 0; EXPECT(sship_pose_set_params(h, &bad) == SSHIP_ERR_INVALID);
    bad = good; bad.abs_tol = -1.0; EXPECT(sship_pose_set_params(h, &bad) == SSHIP_ERR_INVALID);
    bad = good; bad.rel_tol = nan; EXPECT(sship_pose_set_params(h, &bad) == SSHIP_ERR_INVALID);
    bad = good; bad.sigma_px = 0.0; EXPECT(sship_pose_set_params(h, &bad) == SSHIP_ERR_INVALID);
    bad = good; bad.lambda_max = 1e-9; EXPECT(sship_pose_set_params(h, &bad) == SSHIP_ERR_INVALID);
    EXPECT(sship_pose_get_params(h, &got) == SSHIP_OK && std::memcmp(&got, &good, sizeof good.sigma_px * 9) == 0 && got.max_iterations == 100);
    EXPECT(sship_pose_set_camera(h, 0.0, cam[1], cam[2], cam[3], cam[4]) == SSHIP_ERR_INVALID);
    EXPECT(sship_pose_set_camera(h, cam[0], -1.0, cam[2], cam[3], cam[4]) == SSHIP_ERR_INVALID);
    EXPECT(sship_pose_set_camera(h, cam[0], cam[1], cam[2], cam[3], 0.0) == SSHIP_ERR_INVALID);
    EXPECT(sship_pose_set_camera(h, cam[0], cam[1], nan, cam[3], cam[4]) == SSHIP_ERR_INVALID);
    double c5[5] = {0, 0, 0, 0, 0};
    EXPECT(sship_pose_get_camera(h, &c5[0], &c5[1], &c5[2], &c5[3], &c5[4]) == SSHIP_OK && std::memcmp(c5, cam, sizeof c5) == 0);
    int32_t st4[4]; double c2[2]; Pose3x4 po{};
    EXPECT(sship_pose_solve_host(h, pts.data(), ms.data(), nullptr, ps.max_obs() + 1, nullptr, po.data(), st4, c2, nullptr) == SSHIP_ERR_INVALID);
    EXPECT(sship_pose_solve_host(h, pts.data(), ms.data(), nullptr, -1, nullptr, po.data(), st4, c2, nullptr) == SSHIP_ERR_INVALID);
  }
  const PoseSolver::Result again = ps.track(pose0, obs);                              // a second call: the same bits
  EXPECT(again.ok && std::memcmp(again.pose.data(), r.pose.data(), 96) == 0 && again.trials == r.trials && again.cost == r.cost);
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) return 2;
  const int32_t st[4] = {r.n_obs, r.n_inliers, r.trials, r.status};
  const double cost[2] = {r.cost_initial, r.cost};
  std::fwrite(r.pose.data(), 8, 12, fo); std::fwrite(st, 4, 4, fo); std::fwrite(cost, 8, 2, fo);
  if (!inl.empty()) std::fwrite(inl.data(), 1, inl.size(), fo);
  std::fclose(fo);
  std::printf("pose solver host layer: %d observations, %d inliers, %d trials, status %d\n", r.n_obs, r.n_inliers, r.trials, r.status);
  return g_fail ? 1 : 0;
}
