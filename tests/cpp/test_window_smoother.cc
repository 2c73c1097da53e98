// The C++ host layer's window smoother (include/superslam_hip/window_smoother.hpp: superslam_hip::WindowSmoother).
//   no arguments : CPU - the window's bookkeeping (fixed-lag drop, pose_of, in_window), the class's argument validation (false, last_error,
//                  nothing thrown) and the C ABI's argument checks (refused before any device is touched)
//   <in.bin> <out.bin> : GPU - one window through add_keyframe and optimize
//       in.bin  = int32 K | int32 max_obs | int32 n_kf | f64 camera [5] | n_kf x { int64 id | f64 pose [12] | int32 m | m x { int64 landmark | f32 uL, uR, v } }
//       out.bin = f64 pose [n_kf][12] | int32 stats [4] | f64 cost [2]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "superslam_hip/window_smoother.hpp"

using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static int run_cpu() {
  const StereoCalibration K{718.856, 718.856, 607.19, 185.22, 0.537};
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<StereoObs> obs(4, StereoObs{7, 600.0, 560.0, 200.0});
  {
    WindowSmoother ws(K, 3, 4);
    EXPECT(ws.window_count() == 0 && !ws.in_window(0) && ws.pose_of(0) == PoseSolver::identity() && ws.handle() == nullptr);
    Pose3x4 T = PoseSolver::identity();
    for (size_t id = 10; id < 15; ++id) {
      T[11] = static_cast<double>(id);
      EXPECT(ws.add_keyframe(id, T, obs));
    }
    EXPECT(ws.window_count() == 3 && !ws.in_window(10) && !ws.in_window(11) && ws.in_window(12) && ws.in_window(14));   // the fixed lag
    EXPECT(ws.pose_of(13)[11] == 13.0 && ws.pose_of(11) == PoseSolver::identity());
    EXPECT(!ws.add_keyframe(15, T, std::vector<StereoObs>(5)) && ws.last_error().find("max_obs") != std::string::npos && ws.window_count() == 3);
    sship_ba_params p = WindowSmoother::default_params();
    EXPECT(p.sigma_px == 1.0 && p.huber_k2 == 9.0 && p.lambda0 == 1e-5 && p.lambda_max == 1e5 && p.abs_tol == 1e-3 && p.rel_tol == 1e-3 && p.max_iterations == 20);
    EXPECT(ws.set_params(p));
    p.max_iterations = 0; EXPECT(!ws.set_params(p) && ws.params().max_iterations == 20);
    p = WindowSmoother::default_params(); p.abs_tol = -1.0; EXPECT(!ws.set_params(p));
    p = WindowSmoother::default_params(); p.rel_tol = nan; EXPECT(!ws.set_params(p) && ws.last_error().find("NaN") != std::string::npos);
    p = WindowSmoother::default_params(); p.sigma_px = 0.0; EXPECT(!ws.set_params(p));
    p = WindowSmoother::default_params(); p.huber_k2 = std::numeric_limits<double>::infinity(); EXPECT(!ws.set_params(p));
    p = WindowSmoother::default_params(); p.lambda0 = 0.0; EXPECT(!ws.set_params(p));
    p = WindowSmoother::default_params(); p.lambda_max = 1e-9; EXPECT(!ws.set_params(p));
  }
  for (int which = 0; which < 4; ++which) {                                           // a bad camera: refused without a device
    StereoCalibration bad = K;
    if (which == 0) bad.fx = 0.0;
    if (which == 1) bad.fy = -1.0;
    if (which == 2) bad.baseline = 0.0;
    if (which == 3) bad.cx = nan;
    WindowSmoother ws(bad, 3);
    EXPECT(!ws.optimize() && ws.handle() == nullptr && !ws.last_error().empty());
  }
  {
    WindowSmoother one(K, 1), wide(K, 17), none(K, 3, 0), big(K, 3, 2049);
    EXPECT(!one.optimize() && one.last_error().find("window_size") != std::string::npos);
    EXPECT(!wide.optimize() && wide.last_error().find("window_size") != std::string::npos);
    EXPECT(!none.optimize() && none.last_error().find("max_obs") != std::string::npos);
    EXPECT(!big.optimize() && big.last_error().find("max_obs") != std::string::npos);
  }
  sship_ba* out = nullptr;
  EXPECT(sship_ba_create(1, 16, 32, 1, &out) == SSHIP_ERR_INVALID && out == nullptr && sship_ba_create(17, 16, 32, 1, &out) == SSHIP_ERR_INVALID);
  EXPECT(sship_ba_create(4, 0, 32, 1, &out) == SSHIP_ERR_INVALID && sship_ba_create(4, 2049, 32, 1, &out) == SSHIP_ERR_INVALID);
  EXPECT(sship_ba_create(4, 16, 0, 1, &out) == SSHIP_ERR_INVALID && sship_ba_create(4, 16, 32769, 1, &out) == SSHIP_ERR_INVALID);
  EXPECT(sship_ba_create(4, 16, 64, 0, &out) == SSHIP_ERR_INVALID && sship_ba_create(4, 16, 64, 65536, &out) == SSHIP_ERR_INVALID);
  EXPECT(sship_ba_create(4, 16, 64, 1, nullptr) == SSHIP_ERR_INVALID);
  sship_ba_params p = WindowSmoother::default_params();
  double d = 0.0; float f = 0.f; int32_t st[4]; uint8_t u = 0;
  EXPECT(sship_ba_set_camera(nullptr, 1, 1, 0, 0, 1) == SSHIP_ERR_INVALID && sship_ba_get_camera(nullptr, &d, &d, &d, &d, &d) == SSHIP_ERR_INVALID);
  EXPECT(sship_ba_set_params(nullptr, &p) == SSHIP_ERR_INVALID && sship_ba_get_params(nullptr, &p) == SSHIP_ERR_INVALID);
  EXPECT(sship_ba_solve_batch_device(nullptr, &f, st, nullptr, &d, 1, &d, st, &d, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_ba_solve_host(nullptr, &f, st, 2, &d, &d, st, &d, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_ba_tracks_from_matches_batch_device(nullptr, &u, st, st, nullptr, 1, st, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_ba_bench(nullptr, 1, &f) == SSHIP_ERR_INVALID);
  sship_ba_destroy(nullptr);
  std::printf(g_fail ? "window smoother host layer: %d check(s) failed (cpu)\n" : "window smoother host layer: all checks passed (cpu)\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return run_cpu();
  std::FILE* fi = std::fopen(argv[1], "rb");
  if (!fi) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int32_t hdr[3] = {0, 0, 0};
  double cam[5];
  if (std::fread(hdr, 4, 3, fi) != 3 || std::fread(cam, 8, 5, fi) != 5) return 2;
  const int K = hdr[0], N = hdr[1], n_kf = hdr[2];
  if (K < 2 || K > 16 || N < 1 || N > 2048 || n_kf < 0 || n_kf > K) return 2;
  WindowSmoother ws(StereoCalibration{cam[0], cam[1], cam[2], cam[3], cam[4]}, static_cast<size_t>(K), N);
  std::vector<size_t> ids;
  std::vector<Pose3x4> start;
  for (int k = 0; k < n_kf; ++k) {
    int64_t id = 0;
    Pose3x4 T{};
    int32_t m = 0;
    if (std::fread(&id, 8, 1, fi) != 1 || std::fread(T.data(), 8, 12, fi) != 12 || std::fread(&m, 4, 1, fi) != 1 || m < 0 || m > N) return 2;
    std::vector<StereoObs> obs(static_cast<size_t>(m));
    for (StereoObs& o : obs) {
      int64_t l = 0;
      float uv[3];
      if (std::fread(&l, 8, 1, fi) != 1 || std::fread(uv, 4, 3, fi) != 3) return 2;
      o = StereoObs{static_cast<size_t>(l), uv[0], uv[1], uv[2]};
    }
    EXPECT(ws.add_keyframe(static_cast<size_t>(id), T, obs));
    ids.push_back(static_cast<size_t>(id));
    start.push_back(T);
  }
  std::fclose(fi);
  EXPECT(ws.window_count() == static_cast<size_t>(n_kf));
  const bool ok = ws.optimize();
  EXPECT(ok);
  if (!ok) { std::printf("%s\n", ws.last_error().c_str()); return 1; }
  const WindowSmoother::Report r = ws.report();
  EXPECT(ws.handle() != nullptr);
  if (n_kf > 0) EXPECT(ws.pose_of(ids[0]) == start[0]);                               // slot 0 is the gauge: its bits are kept
  sship_ba_params p = WindowSmoother::default_params();
  p.max_iterations = 0;
  EXPECT(!ws.set_params(p) && ws.params().max_iterations == 20);                      // the class refuses on a live handle too, the old values kept
  {
    sship_ba* h = ws.handle();                                                        // and so does the library underneath the class
    const sship_ba_params good = WindowSmoother::default_params();
    sship_ba_params got = good, bad = good;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    bad = good; bad.max_iterations = 0; EXPECT(sship_ba_set_params(h, &bad) == SSHIP_ERR_INVALID);
    bad = good; bad.abs_tol = -1.0; EXPECT(sship_ba_set_params(h, &bad) == SSHIP_ERR_INVALID);
    bad = good; bad.rel_tol = nan; EXPECT(sship_ba_set_params(h, &bad) == SSHIP_ERR_INVALID);
    bad = good; bad.sigma_px = 0.0; EXPECT(sship_ba_set_params(h, &bad) == SSHIP_ERR_INVALID);
    bad = good; bad.lambda_max = 1e-9; EXPECT(sship_ba_set_params(h, &bad) == SSHIP_ERR_INVALID);
    EXPECT(sship_ba_get_params(h, &got) == SSHIP_OK && std::memcmp(&got, &good, sizeof good.sigma_px * 6) == 0 && got.max_iterations == 20);
    EXPECT(sship_ba_set_camera(h, 0.0, cam[1], cam[2], cam[3], cam[4]) == SSHIP_ERR_INVALID);
    EXPECT(sship_ba_set_camera(h, cam[0], cam[1], nan, cam[3], cam[4]) == SSHIP_ERR_INVALID);
    double c5[5] = {0, 0, 0, 0, 0};
    EXPECT(sship_ba_get_camera(h, &c5[0], &c5[1], &c5[2], &c5[3], &c5[4]) == SSHIP_OK && std::memcmp(c5, cam, sizeof c5) == 0);
  }
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) return 2;
  for (int k = 0; k < n_kf; ++k) { const Pose3x4 T = ws.pose_of(ids[static_cast<size_t>(k)]); std::fwrite(T.data(), 8, 12, fo); }
  const int32_t st[4] = {r.n_obs, r.n_landmarks, r.trials, r.status};
  const double cost[2] = {r.cost_initial, r.cost};
  std::fwrite(st, 4, 4, fo); std::fwrite(cost, 8, 2, fo);
  std::fclose(fo);
  std::printf("window smoother host layer: %d keyframes, %d observations, %d landmarks, %d trials, status %d\n", n_kf, r.n_obs, r.n_landmarks, r.trials, r.status);
  return g_fail ? 1 : 0;
}
