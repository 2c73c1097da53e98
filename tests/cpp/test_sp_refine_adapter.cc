// The reference-side SuperPoint adapter (integration/reference_side/SuperPoint.h) passes the keypoint-refinement mode through: compiled
// against the reference's own headers and the stand-in OpenCV / spdlog declarations of tests/cpp/shim.
//   no arguments : CPU - off unless called, validated and kept before initialize()
//   <sp weights> <pair.bin> <out.bin> <max_kp> <border> : GPU - one stereo extraction in sub-pixel mode through the adapter
//       (file formats: tests/cpp/test_sp_refine.cc)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "SuperPoint.h"

// the reference's logger singleton lives in its src/Logging.cc (spdlog sinks); the stand-in of tests/cpp/test_reference_binding.cc
std::shared_ptr<spdlog::logger> superslam::Logger::logger_;
bool superslam::Logger::initialized_ = false;
void superslam::Logger::initialize() { if (!logger_) logger_ = std::make_shared<spdlog::logger>(); initialized_ = true; }
std::shared_ptr<spdlog::logger> superslam::Logger::getLogger() { if (!logger_) initialize(); return logger_; }

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

int main(int argc, char** argv) {
  if (argc < 6) {
    SuperPoint sp("no_such_file.safetensors", 600, 0.005, 4);
    CHECK(sp.keypoint_refinement() == SSHIP_KP_INTEGER);
    CHECK(sp.set_keypoint_refinement(SSHIP_KP_SUBPIXEL) && sp.keypoint_refinement() == SSHIP_KP_SUBPIXEL);
    CHECK(!sp.set_keypoint_refinement(2));
    CHECK(sp.keypoint_refinement() == SSHIP_KP_SUBPIXEL);
    CHECK(sp.set_keypoint_refinement(SSHIP_KP_INTEGER));
    std::printf(g_fail ? "adapter refinement pass-through: %d check(s) failed\n" : "adapter refinement pass-through: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  }
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) { std::printf("cannot open %s\n", argv[2]); return 2; }
  int32_t hw[2] = {0, 0};
  if (std::fread(hw, 4, 2, f) != 2 || hw[0] <= 0 || hw[1] <= 0) return 2;
  cv::Mat left(hw[0], hw[1], CV_8UC1), right(hw[0], hw[1], CV_8UC1);
  for (cv::Mat* m : {&left, &right})
    for (int y = 0; y < hw[0]; ++y)
      if (std::fread(m->ptr<unsigned char>(y), 1, hw[1], f) != static_cast<size_t>(hw[1])) return 2;
  std::fclose(f);
  SuperPoint sp(argv[1], std::atoi(argv[4]), 0.005, std::atoi(argv[5]));
  CHECK(sp.set_keypoint_refinement(SSHIP_KP_SUBPIXEL));
  CHECK(sp.initialize());
  if (g_fail) return 1;
  auto lr = sp.extract_stereo(left, right);
  std::FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 2;
  const int32_t n[2] = {static_cast<int32_t>(lr.first.keypoints.size()), static_cast<int32_t>(lr.second.keypoints.size())};
  CHECK(n[0] > 0 && n[1] > 0);
  std::fwrite(n, 4, 2, o);
  for (const superslam::Features* ft : {&lr.first, &lr.second}) {
    std::vector<float> kp, d(static_cast<size_t>(ft->descriptors.count) * 256);
    for (const cv::KeyPoint& k : ft->keypoints) { kp.push_back(k.pt.x); kp.push_back(k.pt.y); kp.push_back(k.response); }
    CHECK(ft->descriptors.count == static_cast<int>(ft->keypoints.size()));
    CHECK(sship_desc_to_host(ft->descriptors.data, ft->descriptors.count, 256, d.data()) == SSHIP_OK);
    std::fwrite(kp.data(), 4, kp.size(), o);
    std::fwrite(d.data(), 4, d.size(), o);
  }
  std::fclose(o);
  std::printf("adapter refinement pass-through: %d / %d keypoints in sub-pixel mode\n", n[0], n[1]);
  return g_fail ? 1 : 0;
}
