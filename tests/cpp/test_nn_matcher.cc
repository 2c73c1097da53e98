// The C++ host layer's nearest-neighbour matcher (include/superslam_hip/nn_matcher.hpp: superslam_hip::NNMatcher).
//   no arguments : CPU - defaults, parameter validation before initialize(), empty results from an uninitialised matcher, the C ABI's
//                  argument checks (refused before any device is touched)
//   <in.bin> <out.bin> <max_kp> <ratio> <distance> <mutual> : GPU - one host-descriptor match through the IFeatureMatcher interface
//       in.bin  = int32 n0, n1 | d0 f32 [n0][256] | d1 f32 [n1][256]
//       out.bin = int32 k | k x (int32 queryIdx, int32 trainIdx, f32 distance)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "superslam_hip/nn_matcher.hpp"

using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static int run_cpu() {
  NNMatcher nn(600);
  EXPECT(nn.ratio_threshold() == 0.f && nn.distance_threshold() == 0.f && nn.mutual_check());
  EXPECT(nn.set_params(0.8f, 0.7f, false));
  EXPECT(nn.ratio_threshold() == 0.8f && nn.distance_threshold() == 0.7f && !nn.mutual_check());
  EXPECT(!nn.set_params(1.5f, 0.f, true));
  EXPECT(!nn.set_params(std::nanf(""), 0.f, true));
  EXPECT(!nn.set_params(0.8f, std::nanf(""), true));
  EXPECT(!nn.last_error().empty());
  EXPECT(nn.ratio_threshold() == 0.8f && nn.distance_threshold() == 0.7f && !nn.mutual_check());
  EXPECT(nn.set_params(-1.f, -2.f, true));  // <= 0: off
  IFeatureMatcher* m = &nn;                 // plugs in as the interface
  HostDescriptors h;
  h.rows = 2; h.cols = 256; h.data.assign(512, 0.f);
  std::vector<KeyPoint> kp(2);
  EXPECT(m->match(kp, h, kp, h).matches.empty());                                 // not initialised
  EXPECT(m->match(kp, DeviceDescriptors(), kp, DeviceDescriptors()).matches.empty());
  EXPECT(m->descriptors_to_host(DeviceDescriptors()).empty());
  MatchResult r;
  EXPECT(!nn.match(kp, h, kp, h, r));
  NNMatcher bad(5000);
  EXPECT(!bad.initialize() && !bad.last_error().empty());                          // max_keypoints out of range: refused without a device
  sship_nn* out = nullptr;
  EXPECT(sship_nn_create(0, 1, &out) == SSHIP_ERR_INVALID && out == nullptr);
  EXPECT(sship_nn_create(600, 1, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_nn_set_params(nullptr, 0.f, 0.f, 1) == SSHIP_ERR_INVALID);
  EXPECT(sship_nn_get_params(nullptr, nullptr, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_nn_match_host(nullptr, 1, h.data.data(), 1, h.data.data(), nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_nn_bench(nullptr, 1, nullptr) == SSHIP_ERR_INVALID);
  sship_nn_destroy(nullptr);
  std::printf(g_fail ? "nn matcher host layer: %d check(s) failed (cpu)\n" : "nn matcher host layer: all checks passed (cpu)\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 7) return run_cpu();
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int32_t n[2] = {0, 0};
  if (std::fread(n, 4, 2, f) != 2 || n[0] <= 0 || n[1] <= 0) return 2;
  HostDescriptors d0, d1;
  d0.rows = n[0]; d1.rows = n[1]; d0.cols = d1.cols = 256;
  d0.data.resize(static_cast<size_t>(n[0]) * 256); d1.data.resize(static_cast<size_t>(n[1]) * 256);
  if (std::fread(d0.data.data(), 4, d0.data.size(), f) != d0.data.size() || std::fread(d1.data.data(), 4, d1.data.size(), f) != d1.data.size()) return 2;
  std::fclose(f);
  NNMatcher nn(std::atoi(argv[3]));
  EXPECT(nn.set_params(static_cast<float>(std::atof(argv[4])), static_cast<float>(std::atof(argv[5])), std::atoi(argv[6]) != 0));  // kept, applied by initialize()
  EXPECT(nn.initialize());
  if (g_fail) { std::printf("%s\n", nn.last_error().c_str()); return 1; }
  float r = -1.f, t = -1.f; int mu = -1;
  EXPECT(sship_nn_get_params(nn.handle(), &r, &t, &mu) == SSHIP_OK && r == nn.ratio_threshold() && t == nn.distance_threshold() && (mu != 0) == nn.mutual_check());
  EXPECT(!nn.set_params(2.f, 0.f, true) && nn.ratio_threshold() == r);
  IFeatureMatcher* m = &nn;
  std::vector<KeyPoint> kp0(n[0]), kp1(n[1]);
  const MatchResult res = m->match(kp0, d0, kp1, d1);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const int32_t k = static_cast<int32_t>(res.matches.size());
  std::fwrite(&k, 4, 1, o);
  for (const DMatch& dm : res.matches) { std::fwrite(&dm.queryIdx, 4, 1, o); std::fwrite(&dm.trainIdx, 4, 1, o); std::fwrite(&dm.distance, 4, 1, o); }
  std::fclose(o);
  std::printf("nn matcher host layer: %d matches of %d x %d\n", k, n[0], n[1]);
  return g_fail ? 1 : 0;
}
