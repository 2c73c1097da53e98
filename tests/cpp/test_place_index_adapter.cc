// The reference-side place-recogniser adapter (integration/reference_side/EigenPlaces.h) with its opt-in device index, compiled against
// the reference's own headers and src/PlaceRecognizer.cc and the stand-in OpenCV / spdlog declarations of tests/cpp/shim.
//   no arguments : CPU - the switch is off by default and the adapter then is the reference's CosineDescriptorIndex, as before
//   <in.bin> <out.bin> <exclude_recent> <top_k> : GPU - the same adds and queries through set_device_index(true) and through the reference's
//       index (switch off, min_score 0.75 = include/EigenPlaces.h:53): ids and score bits must agree; the device path's results go to out.bin
//       (file formats: tests/cpp/test_place_index.cc)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "EigenPlaces.h"

// the reference's logger singleton lives in its src/Logging.cc (spdlog sinks); the stand-in of tests/cpp/test_reference_binding.cc
std::shared_ptr<spdlog::logger> superslam::Logger::logger_;
bool superslam::Logger::initialized_ = false;
void superslam::Logger::initialize() { if (!logger_) logger_ = std::make_shared<spdlog::logger>(); initialized_ = true; }
std::shared_ptr<spdlog::logger> superslam::Logger::getLogger() { if (!logger_) initialize(); return logger_; }

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static cv::Mat row_of(const float* p, int dim) {
  cv::Mat m(1, dim, CV_32F);
  std::memcpy(m.ptr<float>(0), p, static_cast<size_t>(dim) * 4);
  return m;
}

int main(int argc, char** argv) {
  if (argc < 5) {
    // switch off (the default): the reference's own index, no library call - three rows, hand-computed
    EigenPlaces ep("/nonexistent.safetensors", 512, 512);
    CHECK(!ep.device_index());
    superslam::IPlaceRecognizer* r = &ep;
    const float a[4] = {2.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 3.f, 0.f, 0.f}, c[4] = {1.f, 1.f, 1.f, 1.f};
    r->add(10, row_of(a, 4)); r->add(11, row_of(b, 4)); r->add(12, row_of(c, 4));
    std::vector<superslam::LoopCandidate> got = r->query(row_of(a, 4), 1, 5);         // row 12 is too recent; row 11 scores 0 < 0.75
    CHECK(got.size() == 1 && got[0].keyframe_id == 10 && got[0].score == 1.f);
    got = r->query(row_of(a, 4), 3, 5);
    CHECK(got.empty());
    ep.set_device_index(true, 64);
    CHECK(ep.device_index());
    CHECK(r->query(row_of(a, 4), 0, 5).empty());                                      // a switch starts from an empty device index
    ep.set_device_index(false);
    CHECK(!ep.device_index() && r->query(row_of(a, 4), 1, 5).size() == 1);            // the reference's index kept its content
    std::printf(g_fail ? "place index adapter: %d check(s) failed\n" : "place index adapter: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int32_t hdr[3] = {0, 0, 0};
  if (std::fread(hdr, 4, 3, f) != 3 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] <= 0) return 2;
  const int M = hdr[0], dim = hdr[1], Q = hdr[2];
  std::vector<int64_t> ids(static_cast<size_t>(M));
  std::vector<float> rows(static_cast<size_t>(M) * dim), qs(static_cast<size_t>(Q) * dim);
  if (std::fread(ids.data(), 8, ids.size(), f) != ids.size() || std::fread(rows.data(), 4, rows.size(), f) != rows.size() ||
      std::fread(qs.data(), 4, qs.size(), f) != qs.size())
    return 2;
  std::fclose(f);
  const size_t exclude = static_cast<size_t>(std::atoi(argv[3]));
  const int top_k = std::atoi(argv[4]);
  EigenPlaces dev("/nonexistent.safetensors", 512, 512), host("/nonexistent.safetensors", 512, 512);
  dev.set_device_index(true, M + 5);
  superslam::IPlaceRecognizer* rd = &dev;
  superslam::IPlaceRecognizer* rh = &host;
  for (int i = 0; i < M; ++i) {
    const cv::Mat m = row_of(rows.data() + static_cast<size_t>(i) * dim, dim);
    rd->add(static_cast<size_t>(ids[i]), m);
    rh->add(static_cast<size_t>(ids[i]), m);
  }
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  int total = 0;
  for (int j = 0; j < Q; ++j) {
    const cv::Mat q = row_of(qs.data() + static_cast<size_t>(j) * dim, dim);
    const std::vector<superslam::LoopCandidate> a = rd->query(q, exclude, top_k), b = rh->query(q, exclude, top_k);
    CHECK(a.size() == b.size());
    for (size_t i = 0; i < a.size() && i < b.size(); ++i) {
      CHECK(a[i].keyframe_id == b[i].keyframe_id);
      CHECK(std::memcmp(&a[i].score, &b[i].score, 4) == 0);
    }
    const int32_t k = static_cast<int32_t>(a.size());
    std::fwrite(&k, 4, 1, o);
    for (const auto& e : a) { const int64_t id = static_cast<int64_t>(e.keyframe_id); std::fwrite(&id, 8, 1, o); std::fwrite(&e.score, 4, 1, o); }
    total += k;
  }
  std::fclose(o);
  CHECK(total > 0);
  std::printf("place index adapter: %d candidates for %d queries over %d rows, device index == reference index\n", total, Q, M);
  return g_fail ? 1 : 0;
}
