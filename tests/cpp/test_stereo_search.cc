// The C++ host layer's stereo search (include/superslam_hip/stereo_search.hpp: superslam_hip::StereoSearchParams, search_stereo).
//   no arguments : CPU - the function's and the C ABI's argument validation (false, an error text, nothing thrown; refused before any device)
//   gpu <file>   : GPU - one pair from a file the Python test wrote (images, keypoints, and the restatement's outputs on the same pair):
//                  search_stereo gives the same bits.  File: i32 {h, w, n, half_window, min_disparity, max_disparity, uniqueness, lr_check},
//                  f32 {min_texture, max_rms}, left [h, w] u8, right [h, w] u8, keypoints [n, 3] f32, then the expected stereo [n, 3] f32,
//                  has_depth [n] u8, status [n] u8 and cost [n] i64.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "superslam_hip/stereo_search.hpp"
using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static constexpr int H = 24, W = 48;

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

static int run_cpu() {
  std::vector<uint8_t> img(H * W, 9), hdo, st;
  std::vector<float> kp{20.f, 12.f, 0.5f, 30.f, 12.f, 0.5f}, so;
  std::vector<int64_t> cost;
  std::string err;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  StereoSearchParams ok;
  EXPECT(ok.half_window == 5 && ok.min_disparity == 0 && ok.max_disparity == 128 && ok.uniqueness == 10 && ok.min_texture == 0.f &&
         ok.max_rms == 0.f && ok.lr_check == 1);
  auto call = [&](const StereoSearchParams& p, const uint8_t* l = nullptr, int ls = W, int h = H, int w = W) {
    err.clear();
    return search_stereo(l ? l : img.data(), ls, img.data(), W, h, w, kp, 3, p, so, hdo, &st, &cost, &err);
  };
  StereoSearchParams p = ok;
  p.half_window = 0; EXPECT(!call(p) && has(err, "half_window"));
  p.half_window = 8; EXPECT(!call(p) && has(err, "half_window"));
  p = ok; p.min_disparity = -1; EXPECT(!call(p) && has(err, "min_disparity"));
  p = ok; p.min_disparity = 129; EXPECT(!call(p) && has(err, "min_disparity"));
  p = ok; p.min_disparity = 127; EXPECT(!call(p) && has(err, "[3, 512]"));
  p = ok; p.max_disparity = 512; EXPECT(!call(p) && has(err, "[3, 512]"));
  p = ok; p.uniqueness = -1; EXPECT(!call(p) && has(err, "uniqueness"));
  p.uniqueness = 100; EXPECT(!call(p) && has(err, "uniqueness"));
  p = ok; p.lr_check = -2; EXPECT(!call(p) && has(err, "lr_check"));
  p.lr_check = 17; EXPECT(!call(p) && has(err, "lr_check"));
  p = ok; p.min_texture = nan; EXPECT(!call(p) && has(err, "NaN"));
  p = ok; p.max_rms = nan; EXPECT(!call(p) && has(err, "NaN"));
  EXPECT(!call(ok, img.data(), W - 1) && has(err, "stride"));
  EXPECT(!call(ok, img.data(), W, 0, W) && has(err, "h and w") && !call(ok, img.data(), 16385, H, 16385));
  EXPECT(so.empty() && hdo.empty());   // a failed call leaves the outputs alone
  {
    std::vector<float> odd(5);
    EXPECT(!search_stereo(img.data(), W, img.data(), W, H, W, odd, 3, ok, so, hdo, nullptr, nullptr, &err) && has(err, "kp_stride"));
    EXPECT(!search_stereo(img.data(), W, img.data(), W, H, W, kp, 1, ok, so, hdo, nullptr, nullptr, &err) && has(err, "kp_stride"));
    EXPECT(!search_stereo(img.data(), W, img.data(), W, H, W, kp, 0, ok, so, hdo, nullptr, nullptr, &err) && has(err, "kp_stride"));
    std::vector<float> many(4097 * 2);
    EXPECT(!search_stereo(img.data(), W, img.data(), W, H, W, many, 2, ok, so, hdo, nullptr, nullptr, &err) && has(err, "4096"));
    std::vector<float> none;
    EXPECT(search_stereo(img.data(), W, img.data(), W, H, W, none, 3, ok, so, hdo, &st, &cost, &err) && so.empty() && st.empty());   // n = 0: nothing is touched
    EXPECT(!search_stereo(nullptr, W, img.data(), W, H, W, none, 3, ok, so, hdo, nullptr, nullptr, &err) && has(err, "null"));
  }
  // the C ABI, before any device: host pointers stand in for device ones
  const sship_stereo_search_params c = ok.c();
  int n = 2;
  float sto[6];
  uint8_t hdb[2];
  auto dev = [&](const uint8_t* im, int pairs, int stride, const float* k_in, const int* np, int unit_stride, int max_kp,
                 const sship_stereo_search_params* q, float* s_out, uint8_t* h_out) {
    return sship_stereo_search_batch_device(im, pairs, H, W, stride, k_in, np, unit_stride, max_kp, q, s_out, h_out, nullptr, nullptr, nullptr);
  };
  EXPECT(dev(nullptr, 1, W, kp.data(), &n, 1, 2, &c, sto, hdb) == SSHIP_ERR_INVALID && dev(img.data(), 1, W, nullptr, &n, 1, 2, &c, sto, hdb) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 1, W, kp.data(), nullptr, 1, 2, &c, sto, hdb) == SSHIP_ERR_INVALID && dev(img.data(), 1, W, kp.data(), &n, 1, 2, nullptr, sto, hdb) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 1, W, kp.data(), &n, 1, 2, &c, nullptr, hdb) == SSHIP_ERR_INVALID && dev(img.data(), 1, W, kp.data(), &n, 1, 2, &c, sto, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 0, W, kp.data(), &n, 1, 2, &c, sto, hdb) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 1, W, kp.data(), &n, 3, 2, &c, sto, hdb) == SSHIP_ERR_INVALID && has(sship_last_error(), "unit_stride"));
  EXPECT(dev(img.data(), 1, W, kp.data(), &n, 0, 2, &c, sto, hdb) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 1, W, kp.data(), &n, 1, 0, &c, sto, hdb) == SSHIP_ERR_INVALID && dev(img.data(), 1, W, kp.data(), &n, 1, 4097, &c, sto, hdb) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 1, W - 1, kp.data(), &n, 1, 2, &c, sto, hdb) == SSHIP_ERR_INVALID && has(sship_last_error(), "stride"));
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
  int32_t hdr[8];
  float fl[2];
  std::vector<uint8_t> left, right, want_hd, want_status, got_hd, got_status;
  std::vector<float> kp, want_stereo, got_stereo;
  std::vector<int64_t> want_cost, got_cost;
  bool ok = std::fread(hdr, 4, 8, f) == 8 && std::fread(fl, 4, 2, f) == 2;
  const size_t h = ok ? hdr[0] : 0, w = ok ? hdr[1] : 0, n = ok ? hdr[2] : 0;
  ok = ok && read_n(f, left, h * w) && read_n(f, right, h * w) && read_n(f, kp, n * 3) && read_n(f, want_stereo, n * 3) && read_n(f, want_hd, n) &&
       read_n(f, want_status, n) && read_n(f, want_cost, n);
  std::fclose(f);
  EXPECT(ok && n > 0);
  if (!ok) return g_fail;
  StereoSearchParams p;
  p.half_window = hdr[3]; p.min_disparity = hdr[4]; p.max_disparity = hdr[5]; p.uniqueness = hdr[6]; p.lr_check = hdr[7];
  p.min_texture = fl[0]; p.max_rms = fl[1];
  std::string err;
  EXPECT(search_stereo(left.data(), (int)w, right.data(), (int)w, (int)h, (int)w, kp, 3, p, got_stereo, got_hd, &got_status, &got_cost, &err));
  EXPECT(got_stereo.size() == n * 3 && std::memcmp(got_stereo.data(), want_stereo.data(), n * 12) == 0);
  EXPECT(got_hd == want_hd && got_status == want_status && got_cost == want_cost);
  int found = 0;
  for (uint8_t s : got_status) found += s == SSHIP_SEARCH_STATUS_FOUND;
  EXPECT(found > 0);
  // rows padded to a stride, and keypoints at stride 2: the same bits
  std::vector<uint8_t> lp(h * (w + 3), 0xEE), rp(h * (w + 5), 0xEE);
  for (size_t y = 0; y < h; ++y) { std::memcpy(&lp[y * (w + 3)], &left[y * w], w); std::memcpy(&rp[y * (w + 5)], &right[y * w], w); }
  std::vector<float> xy(n * 2), s2;
  for (size_t i = 0; i < n; ++i) { xy[2 * i] = kp[3 * i]; xy[2 * i + 1] = kp[3 * i + 1]; }
  std::vector<uint8_t> h2;
  EXPECT(search_stereo(lp.data(), (int)w + 3, rp.data(), (int)w + 5, (int)h, (int)w, xy, 2, p, s2, h2, nullptr, nullptr, &err));
  EXPECT(s2.size() == n * 3 && std::memcmp(s2.data(), want_stereo.data(), n * 12) == 0 && h2 == want_hd);
  return g_fail;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 2 && std::strcmp(argv[1], "gpu") == 0;
  const int rc = gpu ? run_gpu(argv[2]) : run_cpu();
  if (rc) { std::printf("%d check(s) failed\n", rc); return 1; }
  std::printf("all checks passed (%s)\n", gpu ? "gpu" : "cpu");
  return 0;
}
