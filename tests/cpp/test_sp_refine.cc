// The C++ host layer's keypoint-refinement pass-through (include/superslam_hip/frontend.hpp: SuperPoint::set_keypoint_refinement).
//   no arguments : CPU - integer by default, a mode set before initialize() is validated and kept, mode 2 is refused
//   <sp weights> <pair.bin> <out.bin> <max_kp> <border> : GPU - one stereo extraction in sub-pixel mode (set BEFORE initialize())
//       pair.bin = int32 h, w | left u8 [h][w] | right u8 [h][w]
//       out.bin  = int32 n_left, n_right | kp_left f32 [n][3] | desc_left f32 [n][256] | kp_right | desc_right
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "superslam_hip/frontend.hpp"

using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static int run_cpu() {
  SuperPoint sp("no_such_file.safetensors", 600, 0.005, 4);
  EXPECT(sp.keypoint_refinement() == SSHIP_KP_INTEGER);
  EXPECT(sp.set_keypoint_refinement(SSHIP_KP_SUBPIXEL));
  EXPECT(sp.keypoint_refinement() == SSHIP_KP_SUBPIXEL);
  EXPECT(!sp.set_keypoint_refinement(2));
  EXPECT(!sp.set_keypoint_refinement(-1));
  EXPECT(!sp.last_error().empty());
  EXPECT(sp.keypoint_refinement() == SSHIP_KP_SUBPIXEL);
  EXPECT(!sp.initialize());  // no such weights file (or no device): the kept mode survives the failed attempt
  EXPECT(sp.keypoint_refinement() == SSHIP_KP_SUBPIXEL);
  EXPECT(sp.set_keypoint_refinement(SSHIP_KP_INTEGER) && sp.keypoint_refinement() == SSHIP_KP_INTEGER);
  EXPECT(sship_sp_set_keypoint_refinement(nullptr, SSHIP_KP_SUBPIXEL) == SSHIP_ERR_INVALID);
  EXPECT(sship_sp_keypoint_refinement(nullptr) == SSHIP_KP_INTEGER);
  std::printf(g_fail ? "refinement pass-through: %d check(s) failed (cpu)\n" : "refinement pass-through: all checks passed (cpu)\n", g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 6) return run_cpu();
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) { std::printf("cannot open %s\n", argv[2]); return 2; }
  int32_t hw[2] = {0, 0};
  if (std::fread(hw, 4, 2, f) != 2 || hw[0] <= 0 || hw[1] <= 0) return 2;
  const size_t px = static_cast<size_t>(hw[0]) * hw[1];
  std::vector<uint8_t> left(px), right(px);
  if (std::fread(left.data(), 1, px, f) != px || std::fread(right.data(), 1, px, f) != px) return 2;
  std::fclose(f);
  SuperPoint sp(argv[1], std::atoi(argv[4]), 0.005, std::atoi(argv[5]));
  EXPECT(sp.set_keypoint_refinement(SSHIP_KP_SUBPIXEL));  // kept and applied by initialize()
  EXPECT(sp.initialize());
  if (g_fail) { std::printf("%s\n", sp.last_error().c_str()); return 1; }
  EXPECT(sship_sp_keypoint_refinement(sp.handle()) == SSHIP_KP_SUBPIXEL);
  EXPECT(!sp.set_keypoint_refinement(2) && sp.keypoint_refinement() == SSHIP_KP_SUBPIXEL);
  Image il{left.data(), hw[0], hw[1], 1, 0}, ir{right.data(), hw[0], hw[1], 1, 0};
  auto lr = sp.extract_stereo(il, ir);
  std::FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 2;
  const int32_t n[2] = {static_cast<int32_t>(lr.first.keypoints.size()), static_cast<int32_t>(lr.second.keypoints.size())};
  EXPECT(n[0] > 0 && n[1] > 0);
  std::fwrite(n, 4, 2, o);
  for (const Features* ft : {&lr.first, &lr.second}) {
    std::vector<float> kp, d(static_cast<size_t>(ft->descriptors.count) * 256);
    for (const KeyPoint& k : ft->keypoints) { kp.push_back(k.x); kp.push_back(k.y); kp.push_back(k.response); }
    EXPECT(ft->descriptors.count == static_cast<int>(ft->keypoints.size()));
    EXPECT(sship_desc_to_host(ft->descriptors.data, ft->descriptors.count, 256, d.data()) == SSHIP_OK);
    std::fwrite(kp.data(), 4, kp.size(), o);
    std::fwrite(d.data(), 4, d.size(), o);
  }
  std::fclose(o);
  std::printf("refinement pass-through: %d / %d keypoints in sub-pixel mode\n", n[0], n[1]);
  return g_fail ? 1 : 0;
}
