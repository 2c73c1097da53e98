// The staging layout of sship_fast_detect_host (csrc/stage_layout.h: FastStage, fast_stage, fast_pack, fast_unpack) alone: no HIP, no
// library.  Built plain and under the host sanitizers by tests/test_fast_cpu.py; a slot that overlaps another, a pack that writes past its
// block or an unpack that reads past it fails here.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../superslam_amd/csrc/stage_layout.h"
using namespace sship;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static void one(int h, int w, int mk, int n_keep, int keep_stride) {
  const FastStage st = fast_stage(h, w, mk);
  const size_t m = (size_t)mk;
  // slots aligned, in order, disjoint
  EXPECT(st.img == 0 && st.n % kStageAlign == 0 && st.keep % kStageAlign == 0 && st.kp % kStageAlign == 0 && st.counts % kStageAlign == 0 &&
         st.carry % kStageAlign == 0);
  EXPECT(st.n >= (size_t)h * w && st.keep >= st.n + 4 && st.in_bytes == st.keep + m * 12 && st.tail_bytes == st.in_bytes - st.n);
  EXPECT(st.counts >= st.kp + m * 12 && st.carry >= st.counts + 8 && st.out_bytes == st.carry + m * 4 && st.rows == m);
  // pack: exactly tail_bytes, the count first, the rows out of strided ones, zeros behind them
  std::vector<float> keep((size_t)n_keep * keep_stride + 1, -5.f);
  for (int i = 0; i < n_keep; ++i)
    for (int k = 0; k < 3; ++k) keep[(size_t)i * keep_stride + k] = 100.f * i + k;
  std::vector<char> tail(st.tail_bytes, 0);
  fast_pack(tail.data(), st, n_keep ? keep.data() : nullptr, keep_stride, n_keep);
  int32_t n32;
  std::memcpy(&n32, tail.data(), 4);
  EXPECT(n32 == n_keep);
  const float* rows = reinterpret_cast<const float*>(tail.data() + (st.keep - st.n));
  for (int i = 0; i < mk; ++i)
    for (int k = 0; k < 3; ++k) EXPECT(rows[3 * i + k] == (i < n_keep ? 100.f * i + k : 0.f));
  // unpack: every byte of the output region lands where it belongs, optional outputs may be absent
  std::vector<char> out(st.out_bytes, 0);
  std::vector<float> kp(m * 3), got(m * 3, -1.f);
  std::vector<int32_t> carry(m), gc(m, -7);
  for (size_t i = 0; i < m * 3; ++i) kp[i] = 0.5f * (float)i;
  for (size_t i = 0; i < m; ++i) carry[i] = (int32_t)i - 3;
  const int32_t counts[2] = {17, 4242};
  std::memcpy(out.data() + st.kp, kp.data(), m * 12);
  std::memcpy(out.data() + st.counts, counts, 8);
  std::memcpy(out.data() + st.carry, carry.data(), m * 4);
  int32_t n_out = -1, n_cand = -1;
  fast_unpack(out.data(), st, got.data(), &n_out, gc.data(), &n_cand);
  EXPECT(got == kp && gc == carry && n_out == 17 && n_cand == 4242);
  n_out = -1;
  fast_unpack(out.data(), st, got.data(), &n_out, nullptr, nullptr);
  EXPECT(n_out == 17);
}

int main() {
  one(7, 7, 1, 0, 3);
  one(7, 7, 1, 1, 3);
  one(16, 12, 8, 5, 3);
  one(45, 83, 64, 64, 5);
  one(376, 1376, 4096, 600, 3);
  one(255, 257, 100, 99, 4);
  if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
  std::printf("all checks passed\n");
  return 0;
}
