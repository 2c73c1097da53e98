// The keypoint-window gate of the reference-side nearest-neighbour adapter (integration/reference_side/NNMatcher.h): compiled against the
// reference's own headers and the stand-in OpenCV / spdlog declarations of tests/cpp/shim.
//   no arguments : CPU - the gate is off by default, validated and kept before initialize()
//   <in.bin> <out.bin> <max_kp> <ratio> <distance> <mutual> <dx_lo> <dx_hi> <dy_lo> <dy_hi> : GPU - one gated cv::Mat match through the
//                  interface, its cv::KeyPoints passed through (file formats: tests/cpp/test_nn_gate_matcher.cc)
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
  if (argc < 11) {
    NNMatcher nn(600);
    CHECK(!nn.gate_enabled());
    CHECK(nn.set_stereo_gate(1.f, 64.f) && nn.gate_enabled());
    CHECK(nn.gate()[0] == 1.f && nn.gate()[1] == 64.f && nn.gate()[2] == -2.f && nn.gate()[3] == 2.f);
    CHECK(!nn.set_gate(std::nanf(""), 1.f, 0.f, 1.f) && !nn.set_gate(2.f, 1.f, 0.f, 1.f) && !nn.set_gate(0.f, 1.f, 2.f, 1.f));
    CHECK(nn.gate_enabled() && nn.gate()[0] == 1.f && nn.gate()[1] == 64.f);
    CHECK(nn.set_gate(-24.f, 24.f, -24.f, 24.f) && nn.gate()[0] == -24.f && nn.gate()[3] == 24.f);
    superslam::IFeatureMatcher* m = &nn;
    cv::Mat d(2, 256, CV_32F);
    std::memset(d.data, 0, 2 * 256 * 4);
    std::vector<cv::KeyPoint> kp(2);
    CHECK(m->match(kp, d, kp, d).matches.empty());
    CHECK(nn.clear_gate() && !nn.gate_enabled());
    std::printf(g_fail ? "nn gate adapter: %d check(s) failed\n" : "nn gate adapter: all checks passed\n", g_fail);
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
  std::vector<cv::KeyPoint> kp0(n[0]), kp1(n[1]);
  for (std::vector<cv::KeyPoint>* kp : {&kp0, &kp1})
    for (cv::KeyPoint& k : *kp) {
      float xy[2];
      if (std::fread(xy, 4, 2, f) != 2) return 2;
      k.pt.x = xy[0]; k.pt.y = xy[1];
    }
  std::fclose(f);
  NNMatcher nn(std::atoi(argv[3]), static_cast<float>(std::atof(argv[4])), static_cast<float>(std::atof(argv[5])), std::atoi(argv[6]) != 0);
  CHECK(nn.set_gate(static_cast<float>(std::atof(argv[7])), static_cast<float>(std::atof(argv[8])), static_cast<float>(std::atof(argv[9])),
                    static_cast<float>(std::atof(argv[10]))));
  CHECK(nn.initialize());
  if (g_fail) return 1;
  superslam::IFeatureMatcher* m = &nn;
  const MatchResult res = m->match(kp0, d0, kp1, d1);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const int32_t k = static_cast<int32_t>(res.matches.size());
  std::fwrite(&k, 4, 1, o);
  for (const cv::DMatch& dm : res.matches) { std::fwrite(&dm.queryIdx, 4, 1, o); std::fwrite(&dm.trainIdx, 4, 1, o); std::fwrite(&dm.distance, 4, 1, o); }
  std::fclose(o);
  std::printf("nn gate adapter: %d matches of %d x %d\n", k, n[0], n[1]);
  return g_fail ? 1 : 0;
}
