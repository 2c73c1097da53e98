// The C++ host layer's patch tracker (include/superslam_hip/patch_tracker.hpp: superslam_hip::PatchTrackParams, track_patches).
//   no arguments : CPU - the function's and the C ABI's argument validation (false, an error text, nothing thrown; refused before any device)
//   gpu <file>   : GPU - one pair from a file the Python test wrote (images, keypoints, predictions, and the restatement's outputs on the
//                  same pair): track_patches gives the same bits.  File: i32 {h, w, n, half_window, search_radius, uniqueness, fb_check,
//                  has_pred}, f32 {min_texture, max_rms}, img0 [h, w] u8, img1 [h, w] u8, keypoints [n, 3] f32, pred [n, 3] f32 (if
//                  has_pred), then the expected kp_out [n, 3] f32, matches0 [n] i32, status [n] u8 and cost [n] i64.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "superslam_hip/patch_tracker.hpp"
using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static constexpr int H = 24, W = 48;

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

static int run_cpu() {
  std::vector<uint8_t> img(H * W, 9), st;
  std::vector<float> kp{20.f, 12.f, 0.5f, 30.f, 12.f, 0.5f}, none, ko;
  std::vector<int32_t> m0;
  std::vector<int64_t> cost;
  std::string err;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  PatchTrackParams ok;
  EXPECT(ok.half_window == 5 && ok.search_radius == 8 && ok.uniqueness == 10 && ok.min_texture == 0.f && ok.max_rms == 0.f && ok.fb_check == 1);
  auto call = [&](const PatchTrackParams& p, const uint8_t* a = nullptr, int s0 = W, int s1 = W, int h = H, int w = W) {
    err.clear();
    return track_patches(a ? a : img.data(), s0, img.data(), s1, h, w, kp, 3, none, 0, p, ko, m0, &st, &cost, &err);
  };
  PatchTrackParams p = ok;
  p.half_window = 0; EXPECT(!call(p) && has(err, "half_window"));
  p.half_window = 8; EXPECT(!call(p) && has(err, "half_window"));
  p = ok; p.search_radius = 0; EXPECT(!call(p) && has(err, "search_radius"));
  p.search_radius = 17; EXPECT(!call(p) && has(err, "search_radius"));
  p = ok; p.uniqueness = -1; EXPECT(!call(p) && has(err, "uniqueness"));
  p.uniqueness = 100; EXPECT(!call(p) && has(err, "uniqueness"));
  p = ok; p.fb_check = -2; EXPECT(!call(p) && has(err, "fb_check"));
  p.fb_check = 17; EXPECT(!call(p) && has(err, "fb_check"));
  p = ok; p.min_texture = nan; EXPECT(!call(p) && has(err, "NaN"));
  p = ok; p.max_rms = nan; EXPECT(!call(p) && has(err, "NaN"));
  EXPECT(!call(ok, img.data(), W - 1) && has(err, "stride"));
  EXPECT(!call(ok, img.data(), W, W - 1) && has(err, "stride"));
  EXPECT(!call(ok, img.data(), W, W, 0, W) && has(err, "h and w") && !call(ok, img.data(), 16385, 16385, H, 16385));
  EXPECT(ko.empty() && m0.empty());   // a failed call leaves the outputs alone
  {
    std::vector<float> odd(5), pr4(4), pr6(6);
    EXPECT(!track_patches(img.data(), W, img.data(), W, H, W, odd, 3, none, 0, ok, ko, m0, nullptr, nullptr, &err) && has(err, "kp_stride"));
    EXPECT(!track_patches(img.data(), W, img.data(), W, H, W, kp, 1, none, 0, ok, ko, m0, nullptr, nullptr, &err) && has(err, "kp_stride"));
    EXPECT(!track_patches(img.data(), W, img.data(), W, H, W, kp, 0, none, 0, ok, ko, m0, nullptr, nullptr, &err) && has(err, "kp_stride"));
    EXPECT(!track_patches(img.data(), W, img.data(), W, H, W, kp, 3, pr4, 3, ok, ko, m0, nullptr, nullptr, &err) && has(err, "pred"));
    EXPECT(!track_patches(img.data(), W, img.data(), W, H, W, kp, 3, pr6, 1, ok, ko, m0, nullptr, nullptr, &err) && has(err, "pred"));
    std::vector<float> many(4097 * 2);
    EXPECT(!track_patches(img.data(), W, img.data(), W, H, W, many, 2, none, 0, ok, ko, m0, nullptr, nullptr, &err) && has(err, "4096"));
    std::vector<float> zero;
    EXPECT(track_patches(img.data(), W, img.data(), W, H, W, zero, 3, none, 0, ok, ko, m0, &st, &cost, &err) && ko.empty() && st.empty());   // n = 0: nothing is touched
    EXPECT(!track_patches(nullptr, W, img.data(), W, H, W, zero, 3, none, 0, ok, ko, m0, nullptr, nullptr, &err) && has(err, "null"));
  }
  // the C ABI, before any device: host pointers stand in for device ones
  const sship_patch_track_params c = ok.c();
  int n = 2;
  float out[6];
  int32_t mb[2];
  auto dev = [&](const uint8_t* i0, long long is0, int s0, const uint8_t* i1, long long is1, int s1, int pairs, const float* k_in, const int* np,
                 int unit_stride, int max_kp, const sship_patch_track_params* q, float* k_out, int32_t* m_out) {
    return sship_patch_track_batch_device(i0, is0, s0, i1, is1, s1, pairs, H, W, k_in, np, unit_stride, nullptr, max_kp, q, k_out, nullptr, m_out,
                                          nullptr, nullptr, nullptr);
  };
  const uint8_t* im = img.data();
  EXPECT(dev(nullptr, 0, W, im, 0, W, 1, kp.data(), &n, 1, 2, &c, out, mb) == SSHIP_ERR_INVALID && dev(im, 0, W, nullptr, 0, W, 1, kp.data(), &n, 1, 2, &c, out, mb) == SSHIP_ERR_INVALID);
  EXPECT(dev(im, 0, W, im, 0, W, 1, nullptr, &n, 1, 2, &c, out, mb) == SSHIP_ERR_INVALID && dev(im, 0, W, im, 0, W, 1, kp.data(), nullptr, 1, 2, &c, out, mb) == SSHIP_ERR_INVALID);
  EXPECT(dev(im, 0, W, im, 0, W, 1, kp.data(), &n, 1, 2, nullptr, out, mb) == SSHIP_ERR_INVALID && dev(im, 0, W, im, 0, W, 1, kp.data(), &n, 1, 2, &c, nullptr, mb) == SSHIP_ERR_INVALID);
  EXPECT(dev(im, 0, W, im, 0, W, 1, kp.data(), &n, 1, 2, &c, out, nullptr) == SSHIP_ERR_INVALID && has(sship_last_error(), "null"));
  EXPECT(dev(im, 0, W, im, 0, W, 0, kp.data(), &n, 1, 2, &c, out, mb) == SSHIP_ERR_INVALID);
  EXPECT(dev(im, 0, W, im, 0, W, 1, kp.data(), &n, 3, 2, &c, out, mb) == SSHIP_ERR_INVALID && has(sship_last_error(), "unit_stride"));
  EXPECT(dev(im, 0, W, im, 0, W, 1, kp.data(), &n, 0, 2, &c, out, mb) == SSHIP_ERR_INVALID);
  EXPECT(dev(im, 0, W, im, 0, W, 1, kp.data(), &n, 1, 0, &c, out, mb) == SSHIP_ERR_INVALID && dev(im, 0, W, im, 0, W, 1, kp.data(), &n, 1, 4097, &c, out, mb) == SSHIP_ERR_INVALID);
  EXPECT(dev(im, 0, W - 1, im, 0, W, 1, kp.data(), &n, 1, 2, &c, out, mb) == SSHIP_ERR_INVALID && has(sship_last_error(), "stride"));
  EXPECT(dev(im, 0, W, im, 0, W - 1, 1, kp.data(), &n, 1, 2, &c, out, mb) == SSHIP_ERR_INVALID && has(sship_last_error(), "stride"));
  EXPECT(dev(im, -1, W, im, 0, W, 1, kp.data(), &n, 1, 2, &c, out, mb) == SSHIP_ERR_INVALID && has(sship_last_error(), "image strides"));
  EXPECT(dev(im, 0, W, im, -1, W, 1, kp.data(), &n, 1, 2, &c, out, mb) == SSHIP_ERR_INVALID && has(sship_last_error(), "image strides"));
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
  std::vector<uint8_t> img0, img1, want_status, got_status;
  std::vector<float> kp, pred, want_kp, got_kp;
  std::vector<int32_t> want_m0, got_m0;
  std::vector<int64_t> want_cost, got_cost;
  bool ok = std::fread(hdr, 4, 8, f) == 8 && std::fread(fl, 4, 2, f) == 2;
  const size_t h = ok ? hdr[0] : 0, w = ok ? hdr[1] : 0, n = ok ? hdr[2] : 0;
  ok = ok && read_n(f, img0, h * w) && read_n(f, img1, h * w) && read_n(f, kp, n * 3) && read_n(f, pred, hdr[7] ? n * 3 : 0) &&
       read_n(f, want_kp, n * 3) && read_n(f, want_m0, n) && read_n(f, want_status, n) && read_n(f, want_cost, n);
  std::fclose(f);
  EXPECT(ok && n > 0);
  if (!ok) return g_fail;
  PatchTrackParams p;
  p.half_window = hdr[3]; p.search_radius = hdr[4]; p.uniqueness = hdr[5]; p.fb_check = hdr[6];
  p.min_texture = fl[0]; p.max_rms = fl[1];
  std::string err;
  EXPECT(track_patches(img0.data(), (int)w, img1.data(), (int)w, (int)h, (int)w, kp, 3, pred, 3, p, got_kp, got_m0, &got_status, &got_cost, &err));
  EXPECT(got_kp.size() == n * 3 && std::memcmp(got_kp.data(), want_kp.data(), n * 12) == 0);
  EXPECT(got_m0 == want_m0 && got_status == want_status && got_cost == want_cost);
  int tracked = 0;
  for (uint8_t s : got_status) tracked += s == SSHIP_TRACK_STATUS_TRACKED;
  EXPECT(tracked > 0);
  // rows padded to a stride, and predictions at stride 2: the same bits
  std::vector<uint8_t> p0(h * (w + 3), 0xEE), p1(h * (w + 5), 0xEE);
  for (size_t y = 0; y < h; ++y) { std::memcpy(&p0[y * (w + 3)], &img0[y * w], w); std::memcpy(&p1[y * (w + 5)], &img1[y * w], w); }
  std::vector<float> pr2(pred.empty() ? 0 : n * 2), k2;
  for (size_t i = 0; i < pr2.size() / 2; ++i) { pr2[2 * i] = pred[3 * i]; pr2[2 * i + 1] = pred[3 * i + 1]; }
  std::vector<int32_t> m2;
  EXPECT(track_patches(p0.data(), (int)w + 3, p1.data(), (int)w + 5, (int)h, (int)w, kp, 3, pr2, 2, p, k2, m2, nullptr, nullptr, &err));
  EXPECT(k2.size() == n * 3 && std::memcmp(k2.data(), want_kp.data(), n * 12) == 0 && m2 == want_m0);
  return g_fail;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 2 && std::strcmp(argv[1], "gpu") == 0;
  const int rc = gpu ? run_gpu(argv[2]) : run_cpu();
  if (rc) { std::printf("%d check(s) failed\n", rc); return 1; }
  std::printf("all checks passed (%s)\n", gpu ? "gpu" : "cpu");
  return 0;
}
