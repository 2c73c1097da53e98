// The C++ host layer's stereo refinement (include/superslam_hip/stereo_refiner.hpp: superslam_hip::StereoRefineParams, refine_stereo).
//   no arguments : CPU - the function's and the C ABI's argument validation (false, an error text, nothing thrown; refused before any device)
//   gpu <file>   : GPU - one pair from a file the Python test wrote (images, keypoints, and the outputs of the batch call on the same pair):
//                  refine_stereo gives the same bits.  File: i32 {h, w, n, half_window, search_radius, on_reject}, f32 {max_rms,
//                  min_disparity}, left [h, w] u8, right [h, w] u8, stereo [n, 3] f32, has_depth [n] u8, then the expected stereo [n, 3],
//                  has_depth [n], status [n] u8 and cost [n] i64.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "superslam_hip/stereo_refiner.hpp"
using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static constexpr int H = 24, W = 48;

static int run_cpu() {
  std::vector<uint8_t> img(H * W, 9), hd{1, 1}, hdo, st;
  std::vector<float> stereo{20.f, 18.f, 12.f, 30.f, 27.f, 12.f}, so;
  std::vector<int64_t> cost;
  std::string err;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  StereoRefineParams ok;
  EXPECT(ok.half_window == 5 && ok.search_radius == 5 && ok.max_rms == 0.f && ok.min_disparity == 0.f && ok.on_reject == SSHIP_REFINE_KEEP);
  auto call = [&](const StereoRefineParams& p, const uint8_t* l = nullptr, int ls = W, int h = H, int w = W) {
    err.clear();
    return refine_stereo(l ? l : img.data(), ls, img.data(), W, h, w, stereo, hd, p, so, hdo, &st, &cost, &err);
  };
  StereoRefineParams p = ok;
  p.half_window = 0; EXPECT(!call(p) && err.find("half_window") != std::string::npos);
  p.half_window = 8; EXPECT(!call(p) && err.find("half_window") != std::string::npos);
  p = ok; p.search_radius = 0; EXPECT(!call(p) && err.find("search_radius") != std::string::npos);
  p.search_radius = 16; EXPECT(!call(p) && err.find("search_radius") != std::string::npos);
  p = ok; p.max_rms = nan; EXPECT(!call(p) && err.find("NaN") != std::string::npos);
  p = ok; p.min_disparity = nan; EXPECT(!call(p) && err.find("NaN") != std::string::npos);
  p = ok; p.on_reject = 2; EXPECT(!call(p) && err.find("on_reject") != std::string::npos);
  EXPECT(!call(ok, img.data(), W - 1) && err.find("stride") != std::string::npos);
  EXPECT(!call(ok, img.data(), W, 0, W) && err.find("h and w") != std::string::npos && !call(ok, img.data(), 16385, H, 16385));
  EXPECT(so.empty() && hdo.empty());   // a failed call leaves the outputs alone
  {
    std::vector<float> odd(5);
    EXPECT(!refine_stereo(img.data(), W, img.data(), W, H, W, odd, hd, ok, so, hdo, nullptr, nullptr, &err) && err.find("3 floats") != std::string::npos);
    std::vector<float> none;
    std::vector<uint8_t> none_hd;
    EXPECT(refine_stereo(img.data(), W, img.data(), W, H, W, none, none_hd, ok, so, hdo, &st, &cost, &err) && so.empty() && st.empty());   // n = 0: nothing is touched
    EXPECT(!refine_stereo(nullptr, W, img.data(), W, H, W, none, none_hd, ok, so, hdo, nullptr, nullptr, &err) && err.find("null") != std::string::npos);
  }
  // the C ABI, before any device: host pointers stand in for device ones
  const sship_stereo_refine_params c = ok.c();
  int n = 2;
  float sto[6];
  uint8_t hdb[2];
  auto dev = [&](const uint8_t* im, int pairs, int stride, const float* s_in, const int* np, int n_stride, int max_kp, const sship_stereo_refine_params* q,
                 float* s_out) {
    return sship_stereo_refine_batch_device(im, pairs, H, W, stride, s_in, hd.data(), np, n_stride, max_kp, q, s_out, hdb, nullptr, nullptr, nullptr);
  };
  EXPECT(dev(nullptr, 1, W, stereo.data(), &n, 1, 2, &c, sto) == SSHIP_ERR_INVALID && dev(img.data(), 1, W, nullptr, &n, 1, 2, &c, sto) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 1, W, stereo.data(), nullptr, 1, 2, &c, sto) == SSHIP_ERR_INVALID && dev(img.data(), 1, W, stereo.data(), &n, 1, 2, nullptr, sto) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 1, W, stereo.data(), &n, 1, 2, &c, nullptr) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 0, W, stereo.data(), &n, 1, 2, &c, sto) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 1, W, stereo.data(), &n, 3, 2, &c, sto) == SSHIP_ERR_INVALID && std::string(sship_last_error()).find("n_stride") != std::string::npos);
  EXPECT(dev(img.data(), 1, W, stereo.data(), &n, 0, 2, &c, sto) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 1, W, stereo.data(), &n, 1, 0, &c, sto) == SSHIP_ERR_INVALID && dev(img.data(), 1, W, stereo.data(), &n, 1, 4097, &c, sto) == SSHIP_ERR_INVALID);
  EXPECT(dev(img.data(), 1, W - 1, stereo.data(), &n, 1, 2, &c, sto) == SSHIP_ERR_INVALID && std::string(sship_last_error()).find("stride") != std::string::npos);
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
  float fl[2];
  std::vector<uint8_t> left, right, hd, want_hd, want_status, got_hd, got_status;
  std::vector<float> stereo, want_stereo, got_stereo;
  std::vector<int64_t> want_cost, got_cost;
  bool ok = std::fread(hdr, 4, 6, f) == 6 && std::fread(fl, 4, 2, f) == 2;
  const size_t h = ok ? hdr[0] : 0, w = ok ? hdr[1] : 0, n = ok ? hdr[2] : 0;
  ok = ok && read_n(f, left, h * w) && read_n(f, right, h * w) && read_n(f, stereo, n * 3) && read_n(f, hd, n) && read_n(f, want_stereo, n * 3) &&
       read_n(f, want_hd, n) && read_n(f, want_status, n) && read_n(f, want_cost, n);
  std::fclose(f);
  EXPECT(ok && n > 0);
  if (!ok) return g_fail;
  StereoRefineParams p;
  p.half_window = hdr[3]; p.search_radius = hdr[4]; p.on_reject = hdr[5]; p.max_rms = fl[0]; p.min_disparity = fl[1];
  std::string err;
  EXPECT(refine_stereo(left.data(), (int)w, right.data(), (int)w, (int)h, (int)w, stereo, hd, p, got_stereo, got_hd, &got_status, &got_cost, &err));
  EXPECT(got_stereo.size() == n * 3 && std::memcmp(got_stereo.data(), want_stereo.data(), n * 12) == 0);
  EXPECT(got_hd == want_hd && got_status == want_status && got_cost == want_cost);
  int refined = 0;
  for (uint8_t s : got_status) refined += s == SSHIP_REFINE_STATUS_REFINED;
  EXPECT(refined > 0);
  // rows padded to a stride: the same bits
  std::vector<uint8_t> lp(h * (w + 3), 0xEE), rp(h * (w + 5), 0xEE);
  for (size_t y = 0; y < h; ++y) { std::memcpy(&lp[y * (w + 3)], &left[y * w], w); std::memcpy(&rp[y * (w + 5)], &right[y * w], w); }
  std::vector<float> s2;
  std::vector<uint8_t> h2;
  EXPECT(refine_stereo(lp.data(), (int)w + 3, rp.data(), (int)w + 5, (int)h, (int)w, stereo, hd, p, s2, h2, nullptr, nullptr, &err));
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
