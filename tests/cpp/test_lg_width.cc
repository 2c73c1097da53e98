// The C++ host layer's adaptive-width pass-throughs (include/superslam_hip/frontend.hpp: LightGlue::set_width_confidence / prune_counts).
//   no arguments : CPU - the setting is validated before initialize() and prune_counts fails softly on an uninitialised matcher
//   <lg weights> <pair.bin> <out.bin> <width> <height> <width_confidence> : GPU - one host-descriptor match with the option on;
//       pair.bin = int32 n0, n1 | f32 kp0 [n0][2] | desc0 [n0][256] | kp1 [n1][2] | desc1 [n1][256]
//       out.bin  = int32 prune0 [n0] | prune1 [n1] | matches0 [n0] (rebuilt from the DMatch list, -1 elsewhere)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "superslam_hip/frontend.hpp"

using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static int run_cpu() {
  LightGlue lg("no_such_file.safetensors", 640, 480, 300);
  EXPECT(lg.set_width_confidence(0.5f, 0));
  EXPECT(lg.set_width_confidence(-1.f));
  EXPECT(!lg.set_width_confidence(std::numeric_limits<float>::quiet_NaN(), 0));
  EXPECT(!lg.set_width_confidence(1.5f, 0));
  EXPECT(!lg.set_width_confidence(0.5f, -1));
  EXPECT(!lg.last_error().empty());
  std::vector<int32_t> p0, p1;
  EXPECT(!lg.prune_counts(3, 2, p0, p1));
  EXPECT(p0.size() == 3 && p1.size() == 2);
  std::printf(g_fail ? "width pass-through: %d check(s) failed (cpu)\n" : "width pass-through: all checks passed (cpu)\n", g_fail);
  return g_fail ? 1 : 0;
}

static bool read_all(std::FILE* f, void* dst, size_t bytes) { return std::fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc < 7) return run_cpu();
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) { std::printf("cannot open %s\n", argv[2]); return 2; }
  int32_t n[2] = {0, 0};
  if (!read_all(f, n, sizeof n) || n[0] <= 0 || n[1] <= 0) return 2;
  std::vector<KeyPoint> kp[2];
  HostDescriptors d[2];
  for (int j = 0; j < 2; ++j) {
    std::vector<float> xy(static_cast<size_t>(n[j]) * 2);
    d[j].rows = n[j]; d[j].cols = 256;
    d[j].data.resize(static_cast<size_t>(n[j]) * 256);
    if (!read_all(f, xy.data(), xy.size() * 4) || !read_all(f, d[j].data.data(), d[j].data.size() * 4)) return 2;
    kp[j].resize(n[j]);
    for (int i = 0; i < n[j]; ++i) { kp[j][i].x = xy[2 * i]; kp[j][i].y = xy[2 * i + 1]; }
  }
  std::fclose(f);
  LightGlue lg(argv[1], std::atoi(argv[4]), std::atoi(argv[5]), 600);
  EXPECT(lg.set_width_confidence(static_cast<float>(std::atof(argv[6])), 0));  // kept and applied by initialize()
  EXPECT(lg.initialize());
  if (g_fail) { std::printf("%s\n", lg.last_error().c_str()); return 1; }
  MatchResult r;
  EXPECT(lg.match(kp[0], d[0], kp[1], d[1], r));
  std::vector<int32_t> p0, p1, m0(n[0], -1);
  EXPECT(lg.prune_counts(n[0], n[1], p0, p1));
  for (const DMatch& m : r.matches) m0[m.queryIdx] = m.trainIdx;
  // turning it off again: every keypoint reports 9
  EXPECT(lg.set_width_confidence(-1.f));
  MatchResult r2;
  std::vector<int32_t> q0, q1;
  EXPECT(lg.match(kp[0], d[0], kp[1], d[1], r2) && lg.prune_counts(n[0], n[1], q0, q1));
  for (int32_t v : q0) EXPECT(v == 9);
  EXPECT(r2.matches.size() > r.matches.size());
  std::FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 2;
  std::fwrite(p0.data(), 4, p0.size(), o);
  std::fwrite(p1.data(), 4, p1.size(), o);
  std::fwrite(m0.data(), 4, m0.size(), o);
  std::fclose(o);
  std::printf("width pass-through: %zu matches with the option on, %zu with it off\n", r.matches.size(), r2.matches.size());
  return g_fail ? 1 : 0;
}
