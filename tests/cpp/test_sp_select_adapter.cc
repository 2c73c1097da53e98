// The reference-side SuperPoint adapter (integration/reference_side/SuperPoint.h) passes the keypoint-selection mode through: compiled
// against the reference's own headers and the stand-in OpenCV / spdlog declarations of tests/cpp/shim.
// CPU: off unless called, mode and bucket validated and kept before initialize().
#include <cstdio>

#include "SuperPoint.h"

// the reference's logger singleton lives in its src/Logging.cc (spdlog sinks); the stand-in of tests/cpp/test_reference_binding.cc
std::shared_ptr<spdlog::logger> superslam::Logger::logger_;
bool superslam::Logger::initialized_ = false;
void superslam::Logger::initialize() { if (!logger_) logger_ = std::make_shared<spdlog::logger>(); initialized_ = true; }
std::shared_ptr<spdlog::logger> superslam::Logger::getLogger() { if (!logger_) initialize(); return logger_; }

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

int main() {
  SuperPoint sp("no_such_file.safetensors", 600, 0.005, 4);
  int g = -1;
  CHECK(sp.keypoint_selection(&g) == SSHIP_SELECT_TOPK && g == 32);
  CHECK(sp.set_keypoint_selection(SSHIP_SELECT_BALANCED, 16) && sp.keypoint_selection(&g) == SSHIP_SELECT_BALANCED && g == 16);
  CHECK(!sp.set_keypoint_selection(2, 16));
  CHECK(!sp.set_keypoint_selection(SSHIP_SELECT_BALANCED, 7));
  CHECK(!sp.set_keypoint_selection(SSHIP_SELECT_BALANCED, 65536));
  CHECK(sp.keypoint_selection(&g) == SSHIP_SELECT_BALANCED && g == 16);
  CHECK(sp.set_keypoint_selection(SSHIP_SELECT_BALANCED) && sp.keypoint_selection(&g) == SSHIP_SELECT_BALANCED && g == 32);
  CHECK(sp.set_keypoint_selection(SSHIP_SELECT_TOPK) && sp.keypoint_selection() == SSHIP_SELECT_TOPK);
  CHECK(sp.keypoint_refinement() == SSHIP_KP_INTEGER && sp.descriptor_sampling() == SSHIP_DESC_NEAREST);
  std::printf(g_fail ? "adapter selection pass-through: %d check(s) failed\n" : "adapter selection pass-through: all checks passed\n", g_fail);
  return g_fail ? 1 : 0;
}
