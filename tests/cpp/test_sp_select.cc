// The C++ host layer's keypoint-selection pass-through (include/superslam_hip/frontend.hpp: SuperPoint::set_keypoint_selection).
// CPU: top-k by default, mode and bucket set before initialize() are validated and kept, mode 2 and buckets 7 / 65536 are refused, and the
// C ABI refuses the same arguments and a NULL handle without a device.
#include <cstdio>

#include "superslam_hip/frontend.hpp"

using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

int main() {
  SuperPoint sp("no_such_file.safetensors", 600, 0.005, 4);
  int g = -1;
  EXPECT(sp.keypoint_selection(&g) == SSHIP_SELECT_TOPK && g == 32);
  EXPECT(sp.set_keypoint_selection(SSHIP_SELECT_BALANCED, 24));
  EXPECT(sp.keypoint_selection(&g) == SSHIP_SELECT_BALANCED && g == 24);
  EXPECT(!sp.set_keypoint_selection(2, 24));
  EXPECT(!sp.set_keypoint_selection(-1, 24));
  EXPECT(!sp.set_keypoint_selection(SSHIP_SELECT_BALANCED, 7));
  EXPECT(!sp.set_keypoint_selection(SSHIP_SELECT_BALANCED, 65536));
  EXPECT(!sp.last_error().empty());
  EXPECT(sp.keypoint_selection(&g) == SSHIP_SELECT_BALANCED && g == 24);
  EXPECT(sp.set_keypoint_selection(SSHIP_SELECT_BALANCED, 8) && sp.keypoint_selection(&g) == SSHIP_SELECT_BALANCED && g == 8);
  EXPECT(sp.set_keypoint_selection(SSHIP_SELECT_BALANCED, 65535) && sp.keypoint_selection(&g) == SSHIP_SELECT_BALANCED && g == 65535);
  EXPECT(!sp.initialize());  // no such weights file (or no device): the kept mode survives the failed attempt
  EXPECT(sp.keypoint_selection(&g) == SSHIP_SELECT_BALANCED && g == 65535);
  EXPECT(sp.set_keypoint_selection(SSHIP_SELECT_TOPK, 3));  // the bucket is ignored for top-k, and the kept one stays
  EXPECT(sp.keypoint_selection(&g) == SSHIP_SELECT_TOPK && g == 65535);
  EXPECT(sp.keypoint_selection() == SSHIP_SELECT_TOPK);
  // the other two modes are untouched
  EXPECT(sp.keypoint_refinement() == SSHIP_KP_INTEGER && sp.descriptor_sampling() == SSHIP_DESC_NEAREST);
  // the C ABI, without a device
  EXPECT(sship_sp_set_keypoint_selection(nullptr, SSHIP_SELECT_BALANCED, 32) == SSHIP_ERR_INVALID);
  EXPECT(sship_sp_set_keypoint_selection(nullptr, SSHIP_SELECT_TOPK, 32) == SSHIP_ERR_INVALID);
  g = -1;
  EXPECT(sship_sp_keypoint_selection(nullptr, &g) == SSHIP_SELECT_TOPK);
  EXPECT(sship_sp_keypoint_selection(nullptr, nullptr) == SSHIP_SELECT_TOPK);
  float buf[4] = {0.f, 0.f, 0.f, 0.f};
  int ibuf[4] = {0, 0, 0, 0};
  EXPECT(sship_select_topk_balanced(nullptr, 8, 8, 8, 8, 0.0, 0, 4, 32, 1, 1, buf, ibuf, ibuf, ibuf, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_select_topk_balanced(buf, 8, 8, 8, 8, 0.0, 0, 0, 32, 1, 1, buf, ibuf, ibuf, ibuf, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_select_topk_balanced(buf, 8, 8, 8, 8, 0.0, 0, 4, 7, 1, 1, buf, ibuf, ibuf, ibuf, nullptr, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(sship_select_topk_balanced(buf, 8, 8, 8, 8, 0.0, 0, 4, 65536, 1, 1, buf, ibuf, ibuf, ibuf, nullptr, nullptr) == SSHIP_ERR_INVALID);
  std::printf(g_fail ? "selection pass-through: %d check(s) failed (cpu)\n" : "selection pass-through: all checks passed (cpu)\n", g_fail);
  return g_fail ? 1 : 0;
}
