// The reference-side nearest-neighbour adapter (integration/reference_side/NNMatcher.h) as a superslam::IFeatureMatcher: compiled against
// the reference's own headers and the stand-in OpenCV / spdlog declarations of tests/cpp/shim.
//   no arguments : CPU - parameters validated and kept before initialize(), empty results from an uninitialised matcher
//   <in.bin> <out.bin> <max_kp> <ratio> <distance> <mutual> : GPU - one cv::Mat match through the interface (file formats: tests/cpp/test_nn_matcher.cc)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "NNMatcher.h"

// the reference's logger singleton lives in its src/Logging.cc (spdlog sinks); the stand-in of tests/cpp/test_reference_binding.cc
std::shared_ptr<spdlog::logger> superslam::Logger::logger_;
bool superslam::Logger::initialized_ = false;
void superslam::Logger::initialize() { if (!logger_) logger_ = std::make_shared<spdlog::logger>(); initialized_ = true; }
std::shared_ptr<spdlog::logger> superslam::Logger::getLogger() { if (!logger_) initialize(); return logger_; }

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

int main(int argc, char** argv) {
  if (argc < 7) {
    NNMatcher nn(600);
    CHECK(nn.ratio_threshold() == 0.f && nn.distance_threshold() == 0.f && nn.mutual_check());
    CHECK(nn.set_params(0.8f, 0.7f, false) && nn.ratio_threshold() == 0.8f && !nn.mutual_check());
    CHECK(!nn.set_params(1.5f, 0.f, true) && !nn.set_params(0.5f, std::nanf(""), true));
    CHECK(nn.ratio_threshold() == 0.8f && nn.distance_threshold() == 0.7f);
    superslam::IFeatureMatcher* m = &nn;
    cv::Mat d(2, 256, CV_32F);
    std::memset(d.data, 0, 2 * 256 * 4);
    std::vector<cv::KeyPoint> kp(2);
    CHECK(m->match(kp, d, kp, d).matches.empty());
    CHECK(m->match(kp, superslam::DeviceDescriptors(), kp, superslam::DeviceDescriptors()).matches.empty());
    CHECK(m->descriptors_to_host(superslam::DeviceDescriptors()).empty());
    std::printf(g_fail ? "nn adapter: %d check(s) failed\n" : "nn adapter: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int32_t n[2] = {0, 0};
  if (std::fread(n, 4, 2, f) != 2 || n[0] <= 0 || n[1] <= 0) return 2;
  cv::Mat d0(n[0], 256, CV_32F), d1(n[1], 256, CV_32F);
  for (cv::Mat* m : {&d0, &d1})
    for (int y = 0; y < m->rows; ++y)
      if (std::fread(m->ptr<float>(y), 4, 256, f) != 256) return 2;
  std::fclose(f);
  NNMatcher nn(std::atoi(argv[3]), static_cast<float>(std::atof(argv[4])), static_cast<float>(std::atof(argv[5])), std::atoi(argv[6]) != 0);
  CHECK(nn.initialize());
  if (g_fail) return 1;
  superslam::IFeatureMatcher* m = &nn;
  std::vector<cv::KeyPoint> kp0(n[0]), kp1(n[1]);
  const MatchResult res = m->match(kp0, d0, kp1, d1);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const int32_t k = static_cast<int32_t>(res.matches.size());
  std::fwrite(&k, 4, 1, o);
  for (const cv::DMatch& dm : res.matches) { std::fwrite(&dm.queryIdx, 4, 1, o); std::fwrite(&dm.trainIdx, 4, 1, o); std::fwrite(&dm.distance, 4, 1, o); }
  std::fclose(o);
  std::printf("nn adapter: %d matches of %d x %d\n", k, n[0], n[1]);
  return g_fail ? 1 : 0;
}
