// The staging layouts of sship_brief_describe_host and sship_hm_match_host (csrc/stage_layout.h: BriefStage, HmStage and their pack /
// unpack) and the compile-time pattern (csrc/brief_pattern.h) alone: no HIP, no library.  Built plain and under the host sanitizers by
// tests/test_brief_cpu.py; a slot that overlaps another, a pack that writes past its block or an unpack that reads past it fails here.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../superslam_amd/csrc/brief_pattern.h"
#include "../../superslam_amd/csrc/stage_layout.h"
using namespace sship;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static void describe(int h, int w, int n, int kp_stride) {
  const BriefStage st = brief_stage(h, w, n);
  const size_t m = (size_t)(n > 0 ? n : 1);
  EXPECT(st.img == 0 && st.n % kStageAlign == 0 && st.kp % kStageAlign == 0 && st.desc % kStageAlign == 0 && st.status % kStageAlign == 0 &&
         st.bin % kStageAlign == 0);
  EXPECT(st.rows == m && st.n >= (size_t)h * w && st.kp >= st.n + 4 && st.in_bytes == st.kp + m * 12 && st.tail_bytes == st.in_bytes - st.n);
  EXPECT(st.status >= st.desc + m * 32 && st.bin >= st.status + m && st.out_bytes == st.bin + m);
  std::vector<float> kp((size_t)n * kp_stride + 1, -5.f);
  for (int i = 0; i < n; ++i) { kp[(size_t)i * kp_stride] = 10.f * i + 1; kp[(size_t)i * kp_stride + 1] = 10.f * i + 2; }
  std::vector<char> tail(st.tail_bytes, 0);
  brief_pack(tail.data(), st, n ? kp.data() : nullptr, kp_stride, n);
  int32_t n32;
  std::memcpy(&n32, tail.data(), 4);
  EXPECT(n32 == n);
  const float* rows = reinterpret_cast<const float*>(tail.data() + (st.kp - st.n));
  for (int i = 0; i < (int)m; ++i) {
    EXPECT(rows[3 * i] == (i < n ? 10.f * i + 1 : 0.f) && rows[3 * i + 1] == (i < n ? 10.f * i + 2 : 0.f) && rows[3 * i + 2] == 0.f);
  }
  std::vector<char> out(st.out_bytes, 0);
  std::vector<uint32_t> d(m * 8), gd((size_t)n * 8 + 1, 7u);
  std::vector<uint8_t> s(m), b(m), gs((size_t)n + 1, 9), gb((size_t)n + 1, 9);
  for (size_t i = 0; i < m * 8; ++i) d[i] = 0x01010101u * (uint32_t)(i + 1);
  for (size_t i = 0; i < m; ++i) { s[i] = (uint8_t)(i % 3); b[i] = (uint8_t)(i % 32); }
  std::memcpy(out.data() + st.desc, d.data(), m * 32);
  std::memcpy(out.data() + st.status, s.data(), m);
  std::memcpy(out.data() + st.bin, b.data(), m);
  brief_unpack(out.data(), st, n, gd.data(), gs.data(), gb.data());
  EXPECT(std::memcmp(gd.data(), d.data(), (size_t)n * 32) == 0 && gd[(size_t)n * 8] == 7u);
  EXPECT(std::memcmp(gs.data(), s.data(), (size_t)n) == 0 && gs[n] == 9 && std::memcmp(gb.data(), b.data(), (size_t)n) == 0 && gb[n] == 9);
  brief_unpack(out.data(), st, n, gd.data(), nullptr, nullptr);
}

static void match(int mk, int n0, int n1, int st0, int st1, bool with_status) {
  const HmStage st = hm_stage(mk);
  const size_t m = (size_t)mk;
  EXPECT(st.lens == 0 && st.desc % kStageAlign == 0 && st.status % kStageAlign == 0 && st.kp % kStageAlign == 0 && st.m0 % kStageAlign == 0 &&
         st.dist0 % kStageAlign == 0 && st.ms0 % kStageAlign == 0);
  EXPECT(st.desc >= 8 && st.desc1 == st.desc + m * 32 && st.status >= st.desc + 2 * m * 32 && st.status1 == st.status + m &&
         st.kp >= st.status + 2 * m && st.kp1 == st.kp + m * 12 && st.in_bytes == st.kp + 2 * m * 12);
  EXPECT(st.dist0 >= st.m0 + m * 4 && st.ms0 >= st.dist0 + m * 4 && st.out_bytes == st.ms0 + m * 4);
  std::vector<uint32_t> d0((size_t)n0 * 8 + 1), d1((size_t)n1 * 8 + 1);
  std::vector<uint8_t> s0((size_t)n0 + 1), s1((size_t)n1 + 1);
  for (size_t i = 0; i < d0.size(); ++i) d0[i] = (uint32_t)(3 * i + 1);
  for (size_t i = 0; i < d1.size(); ++i) d1[i] = (uint32_t)(5 * i + 2);
  for (size_t i = 0; i < s0.size(); ++i) s0[i] = (uint8_t)(i % 3);
  for (size_t i = 0; i < s1.size(); ++i) s1[i] = (uint8_t)((i + 1) % 3);
  std::vector<float> k0((size_t)n0 * st0 + 1, -5.f), k1((size_t)n1 * st1 + 1, -5.f);
  for (int i = 0; i < n0; ++i) { k0[(size_t)i * st0] = 2.f * i; k0[(size_t)i * st0 + 1] = 2.f * i + 1; }
  for (int i = 0; i < n1; ++i) { k1[(size_t)i * st1] = 7.f * i; k1[(size_t)i * st1 + 1] = 7.f * i + 1; }
  std::vector<char> in(st.in_bytes, 0);
  hm_pack(in.data(), st, n0, n0 ? d0.data() : nullptr, with_status ? s0.data() : nullptr, n1, n1 ? d1.data() : nullptr, with_status ? s1.data() : nullptr);
  hm_pack_kp(in.data(), st, k0.data(), st0, n0, k1.data(), st1, n1);
  int32_t lens[2];
  std::memcpy(lens, in.data() + st.lens, 8);
  EXPECT(lens[0] == n0 && lens[1] == n1);
  EXPECT(std::memcmp(in.data() + st.desc, d0.data(), (size_t)n0 * 32) == 0 && std::memcmp(in.data() + st.desc1, d1.data(), (size_t)n1 * 32) == 0);
  const uint8_t* p0 = reinterpret_cast<const uint8_t*>(in.data() + st.status);
  const uint8_t* p1 = reinterpret_cast<const uint8_t*>(in.data() + st.status1);
  for (int i = 0; i < mk; ++i) {
    EXPECT(p0[i] == (i < n0 ? (with_status ? s0[i] : 1) : 0) && p1[i] == (i < n1 ? (with_status ? s1[i] : 1) : 0));
  }
  const float* q0 = reinterpret_cast<const float*>(in.data() + st.kp);
  const float* q1 = reinterpret_cast<const float*>(in.data() + st.kp1);
  for (int i = 0; i < mk; ++i) {
    EXPECT(q0[3 * i] == (i < n0 ? 2.f * i : 0.f) && q0[3 * i + 1] == (i < n0 ? 2.f * i + 1 : 0.f) && q0[3 * i + 2] == 0.f);
    EXPECT(q1[3 * i] == (i < n1 ? 7.f * i : 0.f) && q1[3 * i + 1] == (i < n1 ? 7.f * i + 1 : 0.f) && q1[3 * i + 2] == 0.f);
  }
  std::vector<char> out(st.out_bytes, 0);
  std::vector<int32_t> a(m), b(m), ga((size_t)n0 + 1, -7), gb((size_t)n0 + 1, -7);
  std::vector<float> c(m), gc((size_t)n0 + 1, -7.f);
  for (size_t i = 0; i < m; ++i) { a[i] = (int32_t)i - 1; b[i] = 256 - (int32_t)i % 257; c[i] = 0.25f * (float)i; }
  std::memcpy(out.data() + st.m0, a.data(), m * 4);
  std::memcpy(out.data() + st.dist0, b.data(), m * 4);
  std::memcpy(out.data() + st.ms0, c.data(), m * 4);
  hm_unpack(out.data(), st, n0, ga.data(), gb.data(), gc.data());
  EXPECT(std::memcmp(ga.data(), a.data(), (size_t)n0 * 4) == 0 && ga[n0] == -7 && std::memcmp(gb.data(), b.data(), (size_t)n0 * 4) == 0 && gb[n0] == -7 &&
         std::memcmp(gc.data(), c.data(), (size_t)n0 * 4) == 0 && gc[n0] == -7.f);
  hm_unpack(out.data(), st, n0, ga.data(), gb.data(), nullptr);
}

// the pattern as the header builds it: the tables' symmetry, the quarter turn, the reach
static void pattern() {
  static constexpr BriefTable tab = make_brief_table();
  static_assert(brief_table_reach(tab) == 14, "reach");
  for (int k = 0; k < kBriefBins; ++k) {
    EXPECT(kBriefSin[k] == kBriefCos[(k + 24) % 32] && kBriefCos[(k + 8) % 32] == -kBriefSin[k] && kBriefSin[(k + 8) % 32] == kBriefCos[k]);
    for (int t = 0; t < kBriefBits; ++t)
      for (int o = 0; o < 4; o += 2) {
        EXPECT(tab.v[(k + 8) % 32][t][o] == -tab.v[k][t][o + 1] && tab.v[(k + 8) % 32][t][o + 1] == tab.v[k][t][o]);
      }
  }
  for (int t = 0; t < kBriefBits; ++t) EXPECT(tab.v[0][t][0] != tab.v[0][t][2] || tab.v[0][t][1] != tab.v[0][t][3]);
  EXPECT(brief_rd(8192) == 1 && brief_rd(-8192) == -1 && brief_rd(8191) == 0 && brief_rd(-8191) == 0 && brief_rd(-24576) == -2);
}

int main() {
  describe(33, 33, 0, 3);
  describe(33, 33, 1, 2);
  describe(40, 57, 64, 3);
  describe(96, 128, 130, 5);
  describe(376, 1376, 4096, 3);
  match(1, 0, 0, 3, 3, false);
  match(1, 1, 1, 2, 3, true);
  match(130, 129, 63, 3, 2, true);
  match(130, 0, 130, 3, 3, false);
  match(4096, 600, 4096, 5, 3, true);
  pattern();
  if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
  std::printf("all checks passed\n");
  return 0;
}
