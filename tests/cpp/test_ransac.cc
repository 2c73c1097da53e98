// The C++ host layer's RANSAC pose seed (include/superslam_hip/ransac_verifier.hpp: superslam_hip::RansacVerifier).
//   no arguments : CPU - the class's argument validation (ok = false, the identity, last_error, nothing thrown) and the C ABI's argument
//                  checks (refused before any device is touched)
//   <in.bin> <out.bin> : GPU - one pair through RansacVerifier::verify, then through verify_and_track
//       in.bin  = int32 n | int32 num_hypotheses | f64 camera [5] | points f32 [n][3] | meas f32 [n][3]
//       out.bin = f64 pose [12] | int32 stats [4] | f64 cost | u8 inlier [n] | f64 chained pose [12] | int32 chained stats [4]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "superslam_hip/ransac_verifier.hpp"

using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static int run_cpu() {
  const StereoCalibration K{718.856, 718.856, 607.19, 185.22, 0.537};
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::vector<StereoPointObs> obs(4, StereoPointObs{1.0, 0.5, 10.0, 600.0, 560.0, 200.0});
  {
    RansacVerifier rv(K, 3);
    EXPECT(rv.max_obs() == 3 && rv.last_error().empty() && rv.handle() == nullptr);
    const RansacVerifier::Result r = rv.verify(obs);                                  // more observations than max_obs
    EXPECT(!r.ok && r.pose == PoseSolver::identity() && r.best_h == -1 && rv.last_error().find("max_obs") != std::string::npos && rv.handle() == nullptr);
    sship_ransac_params p = RansacVerifier::default_params();
    EXPECT(p.inlier_px == 3.0 && p.min_disparity == 1.0 && p.min_area2 == 1e-8 && p.seed == 1u && p.num_hypotheses == 512);
    EXPECT(rv.set_params(p));
    p.num_hypotheses = 0; EXPECT(!rv.set_params(p) && rv.params().num_hypotheses == 512);
    p = RansacVerifier::default_params(); p.num_hypotheses = 65537; EXPECT(!rv.set_params(p));
    p = RansacVerifier::default_params(); p.inlier_px = -1.0; EXPECT(!rv.set_params(p));
    p = RansacVerifier::default_params(); p.min_disparity = nan; EXPECT(!rv.set_params(p) && rv.last_error().find("NaN") != std::string::npos);
    p = RansacVerifier::default_params(); p.min_area2 = inf; EXPECT(!rv.set_params(p));
    p = RansacVerifier::default_params(); p.min_area2 = -1e-9; EXPECT(!rv.set_params(p));
    p = RansacVerifier::default_params(); p.seed = 0xffffffffu; p.num_hypotheses = 65536; EXPECT(rv.set_params(p) && rv.params().seed == 0xffffffffu);
  }
  for (int which = 0; which < 4; ++which) {                                           // a bad camera: refused without a device
    StereoCalibration bad = K;
    if (which == 0) bad.fx = 0.0;
    if (which == 1) bad.fy = -1.0;
    if (which == 2) bad.baseline = 0.0;
    if (which == 3) bad.cx = nan;
    RansacVerifier rv(bad);
    const RansacVerifier::Result r = rv.verify(obs);
    EXPECT(!r.ok && rv.handle() == nullptr && !rv.last_error().empty());
  }
  {
    RansacVerifier none(K, 0), wide(K, 2049);
    EXPECT(!none.verify(std::vector<StereoPointObs>()).ok && none.last_error().find("max_obs") != std::string::npos);
    EXPECT(!wide.verify(obs).ok && wide.last_error().find("max_obs") != std::string::npos);
  }
  sship_ransac* out = nullptr;
  EXPECT(sship_ransac_create(0, 1, &out) == SSHIP_ERR_INVALID && out == nullptr);
  EXPECT(sship_ransac_create(2049, 1, &out) == SSHIP_ERR_INVALID && sship_ransac_create(16, 0, &out) == SSHIP_ERR_INVALID);
  EXPECT(sship_ransac_create(16, 65536, &out) == SSHIP_ERR_INVALID && sship_ransac_create(16, 1, nullptr) == SSHIP_ERR_INVALID);
  sship_ransac_params p = RansacVerifier::default_params();
  double d = 0.0; float f = 0.f; int32_t st[4]; uint8_t u = 0;
  EXPECT(sship_ransac_set_camera(nullptr, 1, 1, 0, 0, 1) == SSHIP_ERR_INVALID && sship_ransac_get_camera(nullptr, &d, &d, &d, &d, &d) == SSHIP_ERR_INVALID);
  EXPECT(sship_ransac_set_params(nullptr, &p) == SSHIP_ERR_INVALID && sship_ransac_get_params(nullptr, &p) == SSHIP_ERR_INVALID);
  EXPECT(sship_ransac_solve_batch_device(nullptr, &f, &f, &u, 1, &d, st, &d, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_ransac_solve_host(nullptr, &f, &f, &u, 1, &d, st, &d, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_ransac_bench(nullptr, 1, &f) == SSHIP_ERR_INVALID);
  sship_ransac_destroy(nullptr);
  std::printf(g_fail ? "ransac host layer: %d check(s) failed (cpu)\n" : "ransac host layer: all checks passed (cpu)\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return run_cpu();
  std::FILE* fi = std::fopen(argv[1], "rb");
  if (!fi) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int32_t n = 0, hyp = 0;
  double cam[5];
  if (std::fread(&n, 4, 1, fi) != 1 || n < 0 || n > 2048 || std::fread(&hyp, 4, 1, fi) != 1 || std::fread(cam, 8, 5, fi) != 5) return 2;
  std::vector<float> pts(static_cast<size_t>(n) * 3), ms(static_cast<size_t>(n) * 3);
  if (std::fread(pts.data(), 4, pts.size(), fi) != pts.size() || std::fread(ms.data(), 4, ms.size(), fi) != ms.size()) return 2;
  std::fclose(fi);
  std::vector<StereoPointObs> obs(static_cast<size_t>(n));
  for (size_t i = 0; i < obs.size(); ++i) obs[i] = StereoPointObs{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], ms[3 * i], ms[3 * i + 1], ms[3 * i + 2]};
  const StereoCalibration K{cam[0], cam[1], cam[2], cam[3], cam[4]};
  RansacVerifier rv(K, n > 0 ? n : 1);
  sship_ransac_params p = RansacVerifier::default_params();
  p.num_hypotheses = hyp;
  EXPECT(rv.set_params(p));                                                           // before the handle exists: kept for its creation
  std::vector<uint8_t> inl;
  const RansacVerifier::Result r = rv.verify(obs, &inl);
  EXPECT(r.ok);
  if (!r.ok) { std::printf("%s\n", rv.last_error().c_str()); return 1; }
  EXPECT(rv.handle() != nullptr && inl.size() == obs.size());
  {                                                                                   // the class and the library refuse on a live handle, the old values kept
    sship_ransac* h = rv.handle();
    sship_ransac_params bad = p, got = p;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    bad.num_hypotheses = 0; EXPECT(!rv.set_params(bad) && rv.params().num_hypotheses == hyp && sship_ransac_set_params(h, &bad) == SSHIP_ERR_INVALID);
    bad = p; bad.inlier_px = nan; EXPECT(!rv.set_params(bad) && sship_ransac_set_params(h, &bad) == SSHIP_ERR_INVALID);
    bad = p; bad.min_disparity = -1.0; EXPECT(!rv.set_params(bad) && sship_ransac_set_params(h, &bad) == SSHIP_ERR_INVALID);
    EXPECT(sship_ransac_get_params(h, &got) == SSHIP_OK && got.inlier_px == p.inlier_px && got.min_disparity == p.min_disparity &&
           got.min_area2 == p.min_area2 && got.seed == p.seed && got.num_hypotheses == hyp);
    EXPECT(sship_ransac_set_camera(h, 0.0, cam[1], cam[2], cam[3], cam[4]) == SSHIP_ERR_INVALID);
    double c5[5] = {0, 0, 0, 0, 0};
    EXPECT(sship_ransac_get_camera(h, &c5[0], &c5[1], &c5[2], &c5[3], &c5[4]) == SSHIP_OK && std::memcmp(c5, cam, sizeof c5) == 0);
    int32_t st4[4]; double c1; Pose3x4 po{};
    EXPECT(sship_ransac_solve_host(h, pts.data(), ms.data(), nullptr, rv.max_obs() + 1, po.data(), st4, &c1, nullptr) == SSHIP_ERR_INVALID);
    EXPECT(sship_ransac_solve_host(h, pts.data(), ms.data(), nullptr, -1, po.data(), st4, &c1, nullptr) == SSHIP_ERR_INVALID);
  }
  const RansacVerifier::Result again = rv.verify(obs);                                // a second call: the same bits
  EXPECT(again.ok && std::memcmp(again.pose.data(), r.pose.data(), 96) == 0 && again.best_h == r.best_h && again.cost == r.cost);
  PoseSolver ps(K, n > 0 ? n : 1);
  RansacVerifier::Result seed;
  std::vector<uint8_t> chained;
  const PoseSolver::Result t = rv.verify_and_track(ps, obs, &chained, &seed);
  EXPECT(t.ok && seed.ok && std::memcmp(seed.pose.data(), r.pose.data(), 96) == 0 && chained.size() == obs.size());
  for (size_t i = 0; i < chained.size(); ++i) EXPECT(!chained[i] || inl[i]);          // the solver saw the RANSAC inliers only
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) return 2;
  const int32_t st[4] = {r.n_present, r.n_inliers, r.best_h, r.status};
  const int32_t st2[4] = {t.n_obs, t.n_inliers, t.trials, t.status};
  std::fwrite(r.pose.data(), 8, 12, fo); std::fwrite(st, 4, 4, fo); std::fwrite(&r.cost, 8, 1, fo);
  if (!inl.empty()) std::fwrite(inl.data(), 1, inl.size(), fo);
  std::fwrite(t.pose.data(), 8, 12, fo); std::fwrite(st2, 4, 4, fo);
  std::fclose(fo);
  std::printf("ransac host layer: %d observations, %d inliers, hypothesis %d, status %d; chained: %d inliers, status %d\n", r.n_present, r.n_inliers,
              r.best_h, r.status, t.n_inliers, t.status);
  return g_fail ? 1 : 0;
}
