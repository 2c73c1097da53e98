// The reference-side LightGlue adapter (integration/reference_side/LightGlue.h) passes adaptive width through: compiled against the
// reference's own headers and the stand-in OpenCV / spdlog declarations of tests/cpp/shim.  CPU only: the setting is validated and
// kept before initialize(); an uninitialised matcher reports no prune counts.
#include <cstdio>
#include <limits>
#include <vector>

#include "LightGlue.h"

// the reference's logger singleton lives in its src/Logging.cc (spdlog sinks); the stand-in of tests/cpp/test_reference_binding.cc
std::shared_ptr<spdlog::logger> superslam::Logger::logger_;
bool superslam::Logger::initialized_ = false;
void superslam::Logger::initialize() { if (!logger_) logger_ = std::make_shared<spdlog::logger>(); initialized_ = true; }
std::shared_ptr<spdlog::logger> superslam::Logger::getLogger() { if (!logger_) initialize(); return logger_; }

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

int main() {
  LightGlue lg("no_such_file.safetensors", 640, 480);
  CHECK(lg.set_width_confidence(0.99f, 256));
  CHECK(lg.set_width_confidence(-1.f));
  CHECK(!lg.set_width_confidence(std::numeric_limits<float>::quiet_NaN()));
  CHECK(!lg.set_width_confidence(2.f, 0));
  CHECK(!lg.set_width_confidence(0.5f, -3));
  std::vector<int32_t> p0, p1;
  CHECK(!lg.prune_counts(4, 4, p0, p1));
  std::printf(g_fail ? "adapter width pass-through: %d check(s) failed\n" : "adapter width pass-through: all checks passed\n", g_fail);
  return g_fail ? 1 : 0;
}
