// The keypoint-window gate of the C++ host layer's nearest-neighbour matcher (include/superslam_hip/nn_matcher.hpp; include/sship.h
// "Keypoint-window gate").
//   no arguments : CPU - the gate is off by default, kept and validated before initialize(); the C ABI's argument checks (refused before
//                  any device is touched)
//   <in.bin> <out.bin> <max_kp> <ratio> <distance> <mutual> <dx_lo> <dx_hi> <dy_lo> <dy_hi> : GPU - one gated host-descriptor match
//                  through the IFeatureMatcher interface
//       in.bin  = int32 n0, n1 | d0 f32 [n0][256] | d1 f32 [n1][256] | kp0 f32 [n0][2] | kp1 f32 [n1][2]
//       out.bin = int32 k | k x (int32 queryIdx, int32 trainIdx, f32 distance)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "superslam_hip/nn_matcher.hpp"

using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static bool gate_is(const NNMatcher& nn, float a, float b, float c, float d) {
  const float* g = nn.gate();
  return g[0] == a && g[1] == b && g[2] == c && g[3] == d;
}

static int run_cpu() {
  const float nan = std::nanf("");
  NNMatcher nn(600);
  EXPECT(!nn.gate_enabled() && gate_is(nn, -INFINITY, INFINITY, -INFINITY, INFINITY));
  EXPECT(nn.set_stereo_gate(1.f, 64.f));
  EXPECT(nn.gate_enabled() && gate_is(nn, 1.f, 64.f, -2.f, 2.f));
  EXPECT(!nn.set_gate(nan, 1.f, 0.f, 1.f));
  EXPECT(!nn.set_gate(0.f, 1.f, 0.f, nan));
  EXPECT(!nn.set_gate(2.f, 1.f, 0.f, 1.f));
  EXPECT(!nn.set_gate(0.f, 1.f, 3.f, 1.f));
  EXPECT(!nn.last_error().empty());
  EXPECT(nn.gate_enabled() && gate_is(nn, 1.f, 64.f, -2.f, 2.f));                  // unchanged
  EXPECT(nn.set_gate(-24.f, 24.f, -INFINITY, INFINITY) && gate_is(nn, -24.f, 24.f, -INFINITY, INFINITY));
  EXPECT(nn.set_gate(5.f, 5.f, 0.f, 0.f));                                         // lo == hi is a window
  EXPECT(nn.clear_gate() && !nn.gate_enabled());
  EXPECT(nn.set_stereo_gate(1.f, 64.f, 3.f) && gate_is(nn, 1.f, 64.f, -3.f, 3.f));
  IFeatureMatcher* m = &nn;
  HostDescriptors h;
  h.rows = 2; h.cols = 256; h.data.assign(512, 0.f);
  std::vector<KeyPoint> kp(2);
  EXPECT(m->match(kp, h, kp, h).matches.empty());                                  // not initialised
  sship_nn* none = nullptr;
  int on = -1;
  EXPECT(sship_nn_set_gate(none, 1, 0.f, 1.f, 0.f, 1.f) == SSHIP_ERR_INVALID);
  EXPECT(sship_nn_get_gate(none, &on, nullptr, nullptr, nullptr, nullptr) == SSHIP_ERR_INVALID && on == -1);
  std::vector<int32_t> m0(2);
  std::vector<float> ms0(2), k(4, 0.f);
  EXPECT(sship_nn_match_gated_host(none, k.data(), 2, 2, h.data.data(), k.data(), 2, 2, h.data.data(), m0.data(), ms0.data()) == SSHIP_ERR_INVALID);
  EXPECT(sship_nn_match_gated_device(none, k.data(), 2, 2, h.data.data(), k.data(), 2, 2, h.data.data(), m0.data(), ms0.data()) == SSHIP_ERR_INVALID);
  EXPECT(sship_nn_match_gated_batch_device(none, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_stereo_associate_batch_device(nullptr, nullptr, nullptr, 1, 600, 1.f, 2.f, nullptr, nullptr, nullptr) == SSHIP_ERR_INVALID);
  std::printf(g_fail ? "nn gate host layer: %d check(s) failed (cpu)\n" : "nn gate host layer: all checks passed (cpu)\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 11) return run_cpu();
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int32_t n[2] = {0, 0};
  if (std::fread(n, 4, 2, f) != 2 || n[0] <= 0 || n[1] <= 0) return 2;
  HostDescriptors d0, d1;
  d0.rows = n[0]; d1.rows = n[1]; d0.cols = d1.cols = 256;
  d0.data.resize(static_cast<size_t>(n[0]) * 256); d1.data.resize(static_cast<size_t>(n[1]) * 256);
  if (std::fread(d0.data.data(), 4, d0.data.size(), f) != d0.data.size() || std::fread(d1.data.data(), 4, d1.data.size(), f) != d1.data.size()) return 2;
  std::vector<KeyPoint> kp0(n[0]), kp1(n[1]);
  for (std::vector<KeyPoint>* kp : {&kp0, &kp1})
    for (KeyPoint& k : *kp) {
      float xy[2];
      if (std::fread(xy, 4, 2, f) != 2) return 2;
      k.x = xy[0]; k.y = xy[1];
    }
  std::fclose(f);
  NNMatcher nn(std::atoi(argv[3]));
  EXPECT(nn.set_params(static_cast<float>(std::atof(argv[4])), static_cast<float>(std::atof(argv[5])), std::atoi(argv[6]) != 0));
  const float g[4] = {static_cast<float>(std::atof(argv[7])), static_cast<float>(std::atof(argv[8])), static_cast<float>(std::atof(argv[9])),
                      static_cast<float>(std::atof(argv[10]))};
  EXPECT(nn.set_gate(g[0], g[1], g[2], g[3]));  // kept, applied by initialize()
  EXPECT(nn.initialize());
  if (g_fail) { std::printf("%s\n", nn.last_error().c_str()); return 1; }
  int on = 0;
  float r[4] = {0, 0, 0, 0};
  EXPECT(sship_nn_get_gate(nn.handle(), &on, &r[0], &r[1], &r[2], &r[3]) == SSHIP_OK && on == 1 && r[0] == g[0] && r[1] == g[1] && r[2] == g[2] && r[3] == g[3]);
  EXPECT(!nn.set_gate(2.f, 1.f, 0.f, 0.f) && gate_is(nn, g[0], g[1], g[2], g[3]));
  // a plain entry point on a gated handle is refused, never a silent ungated match
  std::vector<int32_t> m0(n[0]);
  std::vector<float> ms0(n[0]);
  EXPECT(sship_nn_match_host(nn.handle(), n[0], d0.data.data(), n[1], d1.data.data(), m0.data(), ms0.data()) == SSHIP_ERR_INVALID);
  IFeatureMatcher* m = &nn;
  const MatchResult res = m->match(kp0, d0, kp1, d1);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const int32_t k = static_cast<int32_t>(res.matches.size());
  std::fwrite(&k, 4, 1, o);
  for (const DMatch& dm : res.matches) { std::fwrite(&dm.queryIdx, 4, 1, o); std::fwrite(&dm.trainIdx, 4, 1, o); std::fwrite(&dm.distance, 4, 1, o); }
  std::fclose(o);
  std::printf("nn gate host layer: %d matches of %d x %d\n", k, n[0], n[1]);
  return g_fail ? 1 : 0;
}
