// The C++ host layer's binary descriptors (include/superslam_hip/binary_descriptor.hpp: describe_brief, brief_pattern, HammingMatcher).
//   no arguments : CPU - the pattern's symmetry, and the functions', the class's and the C ABI's argument validation (false, an error text,
//                  nothing thrown; refused before any device)
//   gpu <file>   : GPU - a file the Python test wrote: one image, keypoints, a second descriptor set and the restatement's outputs.
//                  describe_brief (packed rows and padded ones) and HammingMatcher::match_host give the restatement's bits.
//                  File: i32 {h, w, n, mode, n1, max_distance}, image [h, w] u8, kp [n, 3] f32, expected desc [n, 8] u32, status [n] u8,
//                  bin [n] u8, desc1 [n1, 8] u32, status1 [n1] u8, expected matches0 [n] i32, dist0 [n] i32.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "superslam_hip/binary_descriptor.hpp"
using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static constexpr int H = 40, W = 48, N = 5;

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

static int run_cpu() {
  std::string err;
  std::vector<int8_t> t0, t8;
  EXPECT(brief_pattern(0, t0, &err) && brief_pattern(8, t8, &err) && t0.size() == 1024 && t8.size() == 1024);
  bool quarter = true, reach = true;
  for (int t = 0; t < 256 && t0.size() == 1024 && t8.size() == 1024; ++t)
    for (int o = 0; o < 4; o += 2) {
      quarter = quarter && t8[4 * t + o] == -t0[4 * t + o + 1] && t8[4 * t + o + 1] == t0[4 * t + o];   // bin 8 is bin 0 turned by 90 degrees
      reach = reach && t0[4 * t + o] >= -14 && t0[4 * t + o] <= 14 && t0[4 * t + o + 1] >= -14 && t0[4 * t + o + 1] <= 14;
    }
  EXPECT(quarter && reach);
  EXPECT(!brief_pattern(-1, t0, &err) && has(err, "bin") && !brief_pattern(32, t0, &err) && has(err, "bin") && t0.size() == 1024);
  EXPECT(sship_brief_pattern(0, nullptr) == SSHIP_ERR_INVALID && has(sship_last_error(), "null"));

  std::vector<uint8_t> img(H * W, 9);
  std::vector<float> kp(N * 3, 20.f);
  std::vector<uint32_t> desc;
  auto host = [&](int stride, int h, int w, int n, int kst, BriefMode m, const uint8_t* im, const float* k) {
    err.clear();
    return describe_brief(im, stride, h, w, k, kst, n, m, desc, nullptr, nullptr, &err);
  };
  EXPECT(!host(W, 32, W, N, 3, BriefMode::Steered, img.data(), kp.data()) && has(err, "h and w"));
  EXPECT(!host(W, H, 16385, N, 3, BriefMode::Steered, img.data(), kp.data()) && has(err, "h and w"));
  EXPECT(!host(W - 1, H, W, N, 3, BriefMode::Steered, img.data(), kp.data()) && has(err, "stride"));
  EXPECT(!host(W, H, W, -1, 3, BriefMode::Steered, img.data(), kp.data()) && has(err, "n must"));
  EXPECT(!host(W, H, W, 4097, 3, BriefMode::Steered, img.data(), kp.data()) && has(err, "n must"));
  EXPECT(!host(W, H, W, N, 1, BriefMode::Steered, img.data(), kp.data()) && has(err, "kp_stride"));
  EXPECT(!host(W, H, W, N, 3, static_cast<BriefMode>(2), img.data(), kp.data()) && has(err, "mode"));
  EXPECT(!host(W, H, W, N, 3, BriefMode::Upright, nullptr, kp.data()) && has(err, "null"));
  EXPECT(!host(W, H, W, N, 3, BriefMode::Upright, img.data(), nullptr) && has(err, "null"));
  EXPECT(host(W, H, W, 0, 3, BriefMode::Upright, img.data(), nullptr) && desc.empty());   // nothing to describe: no device needed
  EXPECT(!describe_brief_device(nullptr, 0, W, 1, H, W, kp.data(), nullptr, 1, N, BriefMode::Steered, nullptr, nullptr, nullptr, nullptr, &err) &&
         has(err, "null"));
  int cnt = N;
  uint32_t out[N * 8];
  auto devcall = [&](long long is, int st, int images, int h, int w, int us, int mk, int mode) {
    return sship_brief_describe_batch_device(img.data(), is, st, images, h, w, kp.data(), &cnt, us, mk, mode, out, nullptr, nullptr, nullptr);
  };
  EXPECT(devcall(-1, W, 1, H, W, 1, N, 0) == SSHIP_ERR_INVALID && has(sship_last_error(), "image_stride"));
  EXPECT(devcall(0, W, 0, H, W, 1, N, 0) == SSHIP_ERR_INVALID && has(sship_last_error(), "images"));
  EXPECT(devcall(0, W, 65536, H, W, 1, N, 0) == SSHIP_ERR_INVALID && has(sship_last_error(), "images"));
  EXPECT(devcall(0, W, 1, H, W, 3, N, 0) == SSHIP_ERR_INVALID && has(sship_last_error(), "unit_stride"));
  EXPECT(devcall(0, W, 1, H, W, 1, 0, 0) == SSHIP_ERR_INVALID && has(sship_last_error(), "max_keypoints"));
  EXPECT(devcall(0, W, 1, H, W, 1, 4097, 0) == SSHIP_ERR_INVALID && has(sship_last_error(), "max_keypoints"));
  EXPECT(devcall(0, W, 1, H, W, 1, N, -1) == SSHIP_ERR_INVALID && has(sship_last_error(), "mode"));
  EXPECT(devcall(0, W, 1, 16, W, 1, N, 0) == SSHIP_ERR_INVALID && has(sship_last_error(), "h and w"));

  HammingMatcher m;
  EXPECT(!m.valid());
  EXPECT(!m.create(0) && has(m.error(), "max_keypoints") && !m.create(4097) && has(m.error(), "max_keypoints"));
  EXPECT(!m.create(64, 0) && has(m.error(), "max_pairs") && !m.create(64, 65536) && has(m.error(), "max_pairs") && !m.valid());
  float ms = 0.f;
  std::vector<int32_t> m0;
  HammingParams p;
  EXPECT(!m.set_params(p) && !m.params(&p) && !m.set_gate(0, 1, 0, 1) && !m.clear_gate() && !m.gate(nullptr) && !m.bench(1, &ms));
  EXPECT(!m.match(&cnt, out, nullptr, nullptr, 0, 2, 1, 2, 1, nullptr, nullptr) && has(m.error(), "null"));
  EXPECT(!m.match_host(1, out, nullptr, nullptr, 1, out, nullptr, nullptr, m0) && has(m.error(), "null") && m0.empty());
  EXPECT(sship_hm_create(64, 1, nullptr) == SSHIP_ERR_INVALID && has(sship_last_error(), "null"));
  return g_fail;
}

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static int run_gpu(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) { std::printf("cannot open %s\n", path); return 1; }
  int32_t hdr[6];
  std::vector<uint8_t> img, want_st, want_bin, st1;
  std::vector<float> kp;
  std::vector<uint32_t> want_desc, d1;
  std::vector<int32_t> want_m0, want_dist;
  bool ok = std::fread(hdr, 4, 6, f) == 6;
  const size_t h = ok ? hdr[0] : 0, w = ok ? hdr[1] : 0, n = ok ? hdr[2] : 0, n1 = ok ? hdr[4] : 0;
  ok = ok && read_n(f, img, h * w) && read_n(f, kp, n * 3) && read_n(f, want_desc, n * 8) && read_n(f, want_st, n) && read_n(f, want_bin, n) &&
       read_n(f, d1, n1 * 8) && read_n(f, st1, n1) && read_n(f, want_m0, n) && read_n(f, want_dist, n);
  std::fclose(f);
  EXPECT(ok);
  if (!ok) return g_fail;
  const BriefMode mode = static_cast<BriefMode>(hdr[3]);
  std::string err;
  std::vector<uint32_t> g0, g1;
  std::vector<uint8_t> s0, b0, padded(h * (w + 3), 0xEE);
  EXPECT(describe_brief(img.data(), (int)w, (int)h, (int)w, kp.data(), 3, (int)n, mode, g0, &s0, &b0, &err));
  for (size_t y = 0; y < h; ++y) std::memcpy(&padded[y * (w + 3)], &img[y * w], w);
  EXPECT(describe_brief(padded.data(), (int)w + 3, (int)h, (int)w, kp.data(), 3, (int)n, mode, g1, nullptr, nullptr, &err));
  EXPECT(g0 == want_desc && g1 == want_desc && s0 == want_st && b0 == want_bin);
  HammingMatcher m;
  HammingParams p;
  p.max_distance = hdr[5];
  EXPECT(m.create((int)(n > n1 ? n : n1), 1, p) && m.valid());
  HammingParams q;
  int mk = 0, mp = 0;
  EXPECT(m.params(&q, &mk, &mp) && q.max_distance == p.max_distance && q.ratio_percent == 0 && q.mutual_check && mk == (int)(n > n1 ? n : n1) && mp == 1);
  float ms = -1.f;
  EXPECT(!m.bench(2, &ms) && has(m.error(), "match"));
  std::vector<int32_t> m0, dist;
  std::vector<float> sc;
  EXPECT(m.match_host((int)n, g0.data(), s0.data(), nullptr, (int)n1, d1.data(), st1.data(), nullptr, m0, &dist, &sc));
  EXPECT(m0 == want_m0 && dist == want_dist && sc.size() == n);
  for (size_t i = 0; i < sc.size() && i < dist.size(); ++i) EXPECT(sc[i] == (dist[i] >= 0 ? (256 - dist[i]) / 256.f : 0.f));
  // gated and no keypoints: refused; the open gate with keypoints: the same bits
  HammingMatcher::Gate g;
  EXPECT(m.set_stereo_gate(-1e30f, 1e30f, 1e30f) && m.gate(&g) && g.enabled);
  EXPECT(!m.match_host((int)n, g0.data(), s0.data(), nullptr, (int)n1, d1.data(), st1.data(), nullptr, m0) && has(m.error(), "gate"));
  std::vector<float> kp1(n1 * 3 + 3, 1.f);
  std::vector<int32_t> m1;
  EXPECT(m.match_host((int)n, g0.data(), s0.data(), kp.data(), (int)n1, d1.data(), st1.data(), kp1.data(), m1) && m.clear_gate() && m.gate(&g) && !g.enabled);
  bool finite = true;
  for (float v : kp) finite = finite && v == v && v - v == 0.f;
  if (finite) EXPECT(m1 == want_m0);
  EXPECT(m.bench(2, &ms) && ms >= 0.f);
  return g_fail;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 2 && std::strcmp(argv[1], "gpu") == 0;
  const int rc = gpu ? run_gpu(argv[2]) : run_cpu();
  if (rc) { std::printf("%d check(s) failed\n", rc); return 1; }
  std::printf("all checks passed (%s)\n", gpu ? "gpu" : "cpu");
  return 0;
}
