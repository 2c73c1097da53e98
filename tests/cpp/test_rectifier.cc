// The C++ host layer's rectifier (include/superslam_hip/rectifier.hpp: superslam_hip::Rectifier, superslam_hip::rgbd_associate).
//   -DRECT_HOST_ONLY : the pure host half alone (superslam_amd/csrc/rect_host.h: map builder, fixed-point table, tile boxes), no library:
//                      the build the host sanitizers run.  Checks the identity map, tie rounding, the degenerate entries, that every masked
//                      tap lies inside its tile's box, and the staged / direct choice.
//   no arguments     : CPU - the class's and the C ABI's argument validation (false, last_error, nothing thrown; refused before any device)
//   gpu              : GPU - a shift map through remap (host image in and out) and one RGB-D frame from host arrays
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

#ifdef RECT_HOST_ONLY
#include "../../superslam_amd/csrc/rect_host.h"
using namespace sship;

static void check_boxes(const std::vector<float>& mx, const std::vector<float>& my, int sw, int sh, int dw, int dh, int* staged, int* direct) {
  std::vector<RectEntry> table;
  std::vector<RectTile> tiles;
  rect_device_table(mx.data(), my.data(), sw, sh, dw, dh, table, tiles, staged, direct);
  const int txn = (dw + kRectTileW - 1) / kRectTileW;
  EXPECT((int)tiles.size() == txn * ((dh + kRectTileH - 1) / kRectTileH) && *staged + *direct == (int)tiles.size());
  for (int v = 0; v < dh; ++v)
    for (int u = 0; u < dw; ++u) {
      const RectEntry& e = table[(size_t)v * dw + u];
      const RectTile& t = tiles[(size_t)(v / kRectTileH) * txn + u / kRectTileW];
      const unsigned mask = e.frac_mask >> 10;
      EXPECT(mask < 16);
      for (int k = 0; k < 4; ++k)
        if (mask & (1u << k)) {
          const int x = e.ix + (k & 1), y = e.iy + (k >> 1);
          if (!(x >= t.x0 && x < t.x0 + t.bw && y >= t.y0 && y < t.y0 + t.bh && x >= 0 && x < sw && y >= 0 && y < sh)) { EXPECT(!"tap outside its box"); return; }
        }
      if (!mask) EXPECT(e.ix == -2 && e.iy == -2 && e.frac_mask == 0);
    }
  for (const RectTile& t : tiles) {
    EXPECT(t.direct == ((long long)t.bh * rect_box_pitch(t.bw) > kRectLdsBytes ? 1 : 0));
    EXPECT(rect_box_pitch(t.bw) % 4 == 0 && rect_box_pitch(t.bw) >= t.bw + 3);
  }
}

int main() {
  // identity camera -> identity map, exactly
  const double K[9] = {100, 0, 32, 0, 100, 24, 0, 0, 1};
  std::vector<float> mx(67 * 41), my(67 * 41);
  EXPECT(rect_build_maps(K, nullptr, 0, nullptr, K, 67, 41, mx.data(), my.data()) == 0);
  for (int v = 0; v < 41; ++v)
    for (int u = 0; u < 67; ++u) EXPECT(mx[v * 67 + u] == (float)u && my[v * 67 + u] == (float)v);
  const double Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  EXPECT(rect_build_maps(K, nullptr, 0, nullptr, Z, 4, 4, mx.data(), my.data()) == 1);
  int staged = 0, direct = 0;
  check_boxes(mx, my, 67, 41, 67, 41, &staged, &direct);
  EXPECT(direct == 0 && staged == 2 * 3);
  // a distorted camera with a shifted principal point: borders on every side
  const double D[5] = {-0.45, 0.1, 0.001, -0.002, 0.0}, P[9] = {100, 0, 12, 0, 100, 15, 0, 0, 1};
  EXPECT(rect_build_maps(K, D, 5, nullptr, P, 67, 41, mx.data(), my.data()) == 0);
  check_boxes(mx, my, 64, 48, 67, 41, &staged, &direct);
  // ties to even, negative coordinates, and the degenerate entries
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float tx[8] = {0.515625f /* 16.5 */, 0.546875f /* 17.5 */, -0.015625f /* -0.5 */, -1.03125f /* -33 */, nan, inf, 32768.0f, 32768.5f};
  const float ty[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int32_t ix[8], iy[8];
  uint16_t fr[8];
  rect_fixed_table(tx, ty, 8, ix, iy, fr);
  EXPECT(ix[0] == 0 && fr[0] == 16 && ix[1] == 0 && fr[1] == 18 && ix[2] == 0 && fr[2] == 0 && ix[3] == -2 && fr[3] == 31);
  EXPECT(fr[4] == 0xFFFF && fr[5] == 0xFFFF && fr[6] != 0xFFFF && ix[6] == 32768 && fr[7] == 0xFFFF);
  // a transpose map of a tall source: the boxes of most tiles exceed the LDS budget
  std::vector<float> qx(256 * 256), qy(256 * 256);
  for (int v = 0; v < 256; ++v)
    for (int u = 0; u < 256; ++u) { qx[v * 256 + u] = (float)v * 15.0f; qy[v * 256 + u] = (float)u * 15.0f; }
  qx[5] = nan; qy[77] = -inf; qx[300] = 1e30f;
  check_boxes(qx, qy, 4096, 4096, 256, 256, &staged, &direct);
  EXPECT(direct > 0);
  if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
  std::printf("all checks passed (host)\n");
  return 0;
}
#else
#include "superslam_hip/rectifier.hpp"
using namespace superslam_hip;

static sship_rgbd_params tum1() {
  sship_rgbd_params p{};
  p.fx = 517.306408; p.fy = 516.469215; p.cx = 318.643040; p.cy = 255.313989;
  p.dist[0] = 0.262383; p.dist[1] = -0.953104; p.dist[2] = -0.005358; p.dist[3] = 0.002628; p.dist[4] = 1.163314;
  p.bf = 40.0; p.depth_factor = 5000.0; p.max_depth = 8.0;
  return p;
}

static int run_cpu() {
  const double K[9] = {100, 0, 32, 0, 100, 24, 0, 0, 1}, Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<float> mx, my;
  std::string err;
  EXPECT(Rectifier::build_maps(K, nullptr, 0, nullptr, K, 64, 48, mx, my, &err) && mx.size() == 64u * 48 && mx[65] == 1.f && my[65] == 1.f);
  EXPECT(!Rectifier::build_maps(K, nullptr, 0, nullptr, Z, 64, 48, mx, my, &err) && err.find("singular") != std::string::npos);
  EXPECT(!Rectifier::build_maps(K, nullptr, 3, nullptr, K, 64, 48, mx, my, &err) && err.find("n_dist") != std::string::npos);
  EXPECT(!Rectifier::build_maps(K, nullptr, 4, nullptr, K, 64, 48, mx, my, &err) && err.find("D is NULL") != std::string::npos);
  EXPECT(!Rectifier::build_maps(K, nullptr, 0, nullptr, K, 0, 48, mx, my, &err) && !Rectifier::build_maps(K, nullptr, 0, nullptr, K, 64, 4097, mx, my, &err));
  double Kb[9];
  std::memcpy(Kb, K, sizeof K);
  Kb[0] = 0.0;
  EXPECT(!Rectifier::build_maps(Kb, nullptr, 0, nullptr, K, 64, 48, mx, my, &err) && err.find("fx") != std::string::npos);
  Kb[0] = nan;
  EXPECT(!Rectifier::build_maps(Kb, nullptr, 0, nullptr, K, 64, 48, mx, my, &err));
  // the C ABI, before any device
  sship_rect* h = nullptr;
  EXPECT(sship_rect_create(0, 48, 64, 48, 2, &h) == SSHIP_ERR_INVALID && !h && sship_rect_create(64, 48, 64, 4097, 2, &h) == SSHIP_ERR_INVALID);
  EXPECT(sship_rect_create(64, 48, 64, 48, 3, &h) == SSHIP_ERR_INVALID && sship_rect_create(64, 48, 64, 48, 0, &h) == SSHIP_ERR_INVALID);
  EXPECT(sship_rect_create(64, 48, 64, 48, 2, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_rect_set_maps(nullptr, 0, mx.data(), my.data()) == SSHIP_ERR_INVALID && sship_rect_set_camera(nullptr, 0, K, nullptr, 0, nullptr, K) == SSHIP_ERR_INVALID);
  EXPECT(sship_rect_remap_batch_device(nullptr, nullptr, 1, 64, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_rect_remap_host(nullptr, 0, nullptr, 64, nullptr) == SSHIP_ERR_INVALID);
  float ms = 0.f;
  EXPECT(sship_rect_bench(nullptr, 1, 0, 1, &ms) == SSHIP_ERR_INVALID);
  sship_rect_destroy(nullptr);
  // the class
  Rectifier r(64, 48, 64, 48, 2);
  std::vector<uint8_t> img(64 * 48, 7), out(64 * 48);
  EXPECT(!r.set_camera(2, K, nullptr, 0, nullptr, K) && r.last_error().find("camera") != std::string::npos && r.handle() == nullptr);
  EXPECT(!r.set_maps(0, nullptr, nullptr) && !r.remap(0, nullptr, 64, out.data()) && !r.remap(-1, img.data(), 64, out.data()));
  EXPECT(!r.remap(0, img.data(), 64, out.data()) && r.last_error().find("no maps") != std::string::npos);
  EXPECT(!r.remap_batch_device(nullptr, 1, 64, nullptr));
  Rectifier bad(64, 48, 64, 48, 3);
  EXPECT(!bad.set_camera(0, K, nullptr, 0, nullptr, K) && !bad.last_error().empty());   // refused by the library: cameras, or no device
  // RGB-D: every refusal comes before the device
  const float kp[4] = {10.f, 12.f, 20.f, 22.f};
  std::vector<uint16_t> depth(48 * 64, 5000);
  std::vector<float> und, st;
  std::vector<uint8_t> hd;
  sship_rgbd_params p = tum1();
  EXPECT(rgbd_associate(kp, 2, 0, depth.data(), SSHIP_DEPTH_U16, 48, 64, 128, p, und, st, hd, &err) && und.empty() && st.empty() && hd.empty());
  EXPECT(!rgbd_associate(nullptr, 2, 2, depth.data(), SSHIP_DEPTH_U16, 48, 64, 128, p, und, st, hd, &err) && err.find("null") != std::string::npos);
  EXPECT(!rgbd_associate(kp, 1, 2, depth.data(), SSHIP_DEPTH_U16, 48, 64, 128, p, und, st, hd, &err) && err.find("kp_stride") != std::string::npos);
  EXPECT(!rgbd_associate(kp, 2, 2, depth.data(), 7, 48, 64, 128, p, und, st, hd, &err) && err.find("depth_type") != std::string::npos);
  EXPECT(!rgbd_associate(kp, 2, 2, depth.data(), SSHIP_DEPTH_U16, 48, 64, 126, p, und, st, hd, &err) && err.find("depth_stride") != std::string::npos);
  EXPECT(!rgbd_associate(kp, 2, 2, depth.data(), SSHIP_DEPTH_F32, 48, 64, 258, p, und, st, hd, &err));
  p.fx = 0.0;
  EXPECT(!rgbd_associate(kp, 2, 2, depth.data(), SSHIP_DEPTH_U16, 48, 64, 128, p, und, st, hd, &err) && err.find("fx") != std::string::npos);
  p = tum1(); p.depth_factor = -1.0;
  EXPECT(!rgbd_associate(kp, 2, 2, depth.data(), SSHIP_DEPTH_U16, 48, 64, 128, p, und, st, hd, &err) && err.find("depth_factor") != std::string::npos);
  p = tum1(); p.dist[6] = nan;
  EXPECT(!rgbd_associate(kp, 2, 2, depth.data(), SSHIP_DEPTH_U16, 48, 64, 128, p, und, st, hd, &err) && err.find("dist") != std::string::npos);
  p = tum1();
  int n = 2;
  float sto[6];
  uint8_t hdo[2];
  EXPECT(sship_rgbd_associate_batch_device(nullptr, &n, 1, 2, depth.data(), 0, 48, 64, 128, &p, nullptr, nullptr, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_rgbd_associate_batch_device(kp, &n, 0, 2, depth.data(), 0, 48, 64, 128, &p, nullptr, sto, hdo, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_rgbd_associate_batch_device(kp, &n, 1, 4097, depth.data(), 0, 48, 64, 128, &p, nullptr, sto, hdo, nullptr) == SSHIP_ERR_INVALID);
  return g_fail;
}

static int run_gpu() {
  // a shift by (+2.5, +1): dst(v, u) = (S(v + 1, u + 2) + S(v + 1, u + 3) + 1) >> 1, zero taps past the border
  const int W = 70, H = 37;
  std::vector<float> mx(W * H), my(W * H);
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) { mx[v * W + u] = u + 2.5f; my[v * W + u] = v + 1.f; }
  std::vector<uint8_t> src(H * 80), out(W * H);
  for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)((i * 37 + 11) % 251);
  Rectifier r(W, H, W, H, 1);
  EXPECT(r.set_maps(0, mx.data(), my.data()) && r.handle());
  EXPECT(r.remap(0, src.data(), 80, out.data()));
  int bad = 0;
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) {
      auto S = [&](int y, int x) { return (x >= 0 && x < W && y >= 0 && y < H) ? (int)src[y * 80 + x] : 0; };
      const int want = (16 * 32 * S(v + 1, u + 2) + 16 * 32 * S(v + 1, u + 3) + 512) >> 10;
      bad += want != out[v * W + u];
    }
  EXPECT(bad == 0);
  EXPECT(!r.remap(0, src.data(), 60, out.data()) && r.last_error().find("src_stride") != std::string::npos);
  const double K[9] = {100, 0, 32, 0, 100, 24, 0, 0, 1};
  Rectifier two(W, H, W, H, 2);
  EXPECT(two.set_camera(0, K, nullptr, 0, nullptr, K));
  EXPECT(!two.remap(1, src.data(), 80, out.data()) && two.last_error().find("no maps") != std::string::npos);
  EXPECT(two.remap(0, src.data(), 80, out.data()));
  bad = 0;
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) bad += out[v * W + u] != src[v * 80 + u];
  EXPECT(bad == 0);
  // one RGB-D frame: a keypoint at the principal point stays put, depth 1 m -> uR = u - bf
  sship_rgbd_params p = tum1();
  const float kp[6] = {(float)p.cx, (float)p.cy, 0.f, 10.f, 20.f, 0.f};
  std::vector<uint16_t> depth(480 * 640, 5000);
  depth[20 * 640 + 10] = 0;
  std::vector<float> und, st;
  std::vector<uint8_t> hd;
  std::string err;
  EXPECT(rgbd_associate(kp, 3, 2, depth.data(), SSHIP_DEPTH_U16, 480, 640, 1280, p, und, st, hd, &err));
  EXPECT(und.size() == 4 && st.size() == 6 && hd.size() == 2 && hd[0] == 1 && hd[1] == 0);
  EXPECT(std::fabs(und[0] - kp[0]) < 1e-3f && std::fabs(und[1] - kp[1]) < 1e-3f && std::fabs(st[1] - (st[0] - 40.f)) < 1e-4f && st[2] == und[1]);
  EXPECT(st[4] != st[4] && st[3] == und[2] && std::fabs(und[2] - kp[3]) > 1.f);   // no depth: NaN; the corner keypoint moves by pixels
  return g_fail;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  const int rc = gpu ? run_gpu() : run_cpu();
  if (rc) { std::printf("%d check(s) failed\n", rc); return 1; }
  std::printf("all checks passed (%s)\n", gpu ? "gpu" : "cpu");
  return 0;
}
#endif
