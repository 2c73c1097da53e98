// The C++ host layer's image pyramid (include/superslam_hip/image_pyramid.hpp: superslam_hip::ImagePyramid, PyramidTrackParams,
// track_patches_pyramid).
//   no arguments : CPU - the classes' and the C ABI's argument validation (false, an error text, nothing thrown; refused before any device)
//   gpu <file>   : GPU - a file the Python test wrote: two images, keypoints, predictions, and the restatements' outputs on them.
//                  ImagePyramid::down and a two-image ImagePyramid (its level 0 in device memory obtained from the HIP runtime the library
//                  already loaded) give the restatement's levels; track_patches_pyramid gives the restatement's bits.
//                  File: i32 {h, w, n, levels, coarse_radius, half_window, search_radius, uniqueness, fb_check, has_pred}, f32 {min_texture,
//                  max_rms}, img0 [h, w] u8, img1 [h, w] u8, keypoints [n, 3] f32, pred [n, 3] f32 (if has_pred), then for l = 1 .. levels - 1
//                  the expected level l of both images [2, h_l, w_l] u8, then the expected kp_out [n, 3] f32, matches0 [n] i32, status [n] u8,
//                  cost [n] i64 and levels_tracked [n] u8.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "superslam_hip/image_pyramid.hpp"
using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static constexpr int H = 24, W = 48;

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

static int run_cpu() {
  std::vector<uint8_t> img(H * W, 9), st, lv, down;
  std::vector<float> kp{20.f, 12.f, 0.5f, 30.f, 12.f, 0.5f}, none, ko;
  std::vector<int32_t> m0;
  std::vector<int64_t> cost;
  std::string err;
  PyramidTrackParams ok;
  EXPECT(ok.levels == 3 && ok.coarse_radius == 8 && ok.fine.half_window == 5 && ok.fine.search_radius == 8 && ok.fine.fb_check == 1);
  auto call = [&](const PyramidTrackParams& p, int s0 = W, int s1 = W, int h = H, int w = W) {
    err.clear();
    return track_patches_pyramid(img.data(), s0, img.data(), s1, h, w, kp, 3, none, 0, p, ko, m0, &st, &cost, &lv, &err);
  };
  PyramidTrackParams p = ok;
  p.levels = 0; EXPECT(!call(p) && has(err, "levels"));
  p.levels = 9; EXPECT(!call(p) && has(err, "levels"));
  p = ok; p.coarse_radius = 0; EXPECT(!call(p) && has(err, "coarse_radius"));
  p.coarse_radius = 17; EXPECT(!call(p) && has(err, "coarse_radius"));
  p = ok; p.fine.half_window = 8; EXPECT(!call(p) && has(err, "half_window"));
  p = ok; p.fine.search_radius = 17; EXPECT(!call(p) && has(err, "search_radius"));
  p = ok; p.fine.max_rms = std::numeric_limits<float>::quiet_NaN(); EXPECT(!call(p) && has(err, "NaN"));
  EXPECT(!call(ok, W - 1) && has(err, "stride") && !call(ok, W, W - 1) && has(err, "stride"));
  EXPECT(!call(ok, W, W, 0, W) && has(err, "h and w"));
  EXPECT(ko.empty() && m0.empty());   // a failed call leaves the outputs alone
  std::vector<float> odd(5), pr4(4), zero;
  EXPECT(!track_patches_pyramid(img.data(), W, img.data(), W, H, W, odd, 3, none, 0, ok, ko, m0, nullptr, nullptr, nullptr, &err) && has(err, "kp_stride"));
  EXPECT(!track_patches_pyramid(img.data(), W, img.data(), W, H, W, kp, 3, pr4, 3, ok, ko, m0, nullptr, nullptr, nullptr, &err) && has(err, "pred"));
  EXPECT(track_patches_pyramid(img.data(), W, img.data(), W, H, W, zero, 3, none, 0, ok, ko, m0, &st, &cost, &lv, &err) && ko.empty() && lv.empty());   // n = 0
  EXPECT(!track_patches_pyramid(nullptr, W, img.data(), W, H, W, zero, 3, none, 0, ok, ko, m0, nullptr, nullptr, nullptr, &err) && has(err, "null"));
  EXPECT(!ImagePyramid::down(img.data(), W, 0, W, down, &err) && has(err, "h and w") && down.empty());
  EXPECT(!ImagePyramid::down(img.data(), W - 1, H, W, down, &err) && has(err, "stride"));
  EXPECT(!ImagePyramid::down(nullptr, W, H, W, down, &err) && has(err, "null"));
  ImagePyramid pyr;
  EXPECT(!pyr.valid());
  EXPECT(!pyr.create(0, W, 3, 1) && has(pyr.error(), "h and w") && !pyr.create(H, W, 0, 1) && has(pyr.error(), "levels"));
  EXPECT(!pyr.create(H, W, 9, 1) && !pyr.create(H, W, 3, 0) && has(pyr.error(), "max_images") && !pyr.valid());
  ImagePyramid::Level L;
  EXPECT(!pyr.build(img.data(), 0, W, 1) && has(pyr.error(), "null") && !pyr.level(0, &L) && !pyr.read_level(0, 0, 1, down));
  float ms = 0.f;
  EXPECT(!pyr.bench(1, &ms));
  // the C ABI of the tracker, before any device
  const sship_pyr_track_params c = ok.c();
  int n = 2;
  float out[6];
  int32_t mb[2];
  EXPECT(sship_patch_track_pyramid_batch_device(nullptr, 0, 1, nullptr, 0, 1, 1, kp.data(), &n, 1, nullptr, 2, &c, out, nullptr, mb, nullptr, nullptr, nullptr,
                                                nullptr) == SSHIP_ERR_INVALID && has(sship_last_error(), "null"));
  return g_fail;
}

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

// device memory without a HIP header: the runtime is in the process already (the library links it)
typedef int (*malloc_fn)(void**, size_t);
typedef int (*free_fn)(void*);
typedef int (*memcpy_fn)(void*, const void*, size_t, int);

static int run_gpu(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) { std::printf("cannot open %s\n", path); return 1; }
  int32_t hdr[10];
  float fl[2];
  std::vector<uint8_t> img0, img1, want_status, want_lv, got_status, got_lv;
  std::vector<std::vector<uint8_t>> want_levels;
  std::vector<float> kp, pred, want_kp, got_kp;
  std::vector<int32_t> want_m0, got_m0;
  std::vector<int64_t> want_cost, got_cost;
  bool ok = std::fread(hdr, 4, 10, f) == 10 && std::fread(fl, 4, 2, f) == 2;
  const size_t h = ok ? hdr[0] : 0, w = ok ? hdr[1] : 0, n = ok ? hdr[2] : 0;
  const int levels = ok ? hdr[3] : 0;
  ok = ok && read_n(f, img0, h * w) && read_n(f, img1, h * w) && read_n(f, kp, n * 3) && read_n(f, pred, hdr[9] ? n * 3 : 0);
  std::vector<size_t> lh{h}, lw{w};
  for (int l = 1; ok && l < levels; ++l) {
    lh.push_back((lh.back() + 1) / 2); lw.push_back((lw.back() + 1) / 2);
    want_levels.emplace_back();
    ok = read_n(f, want_levels.back(), 2 * lh[l] * lw[l]);
  }
  ok = ok && read_n(f, want_kp, n * 3) && read_n(f, want_m0, n) && read_n(f, want_status, n) && read_n(f, want_cost, n) && read_n(f, want_lv, n);
  std::fclose(f);
  EXPECT(ok && n > 0 && levels >= 2);
  if (!ok || levels < 2) return g_fail;
  std::string err;
  // one reduction from host arrays, packed and with padded rows
  std::vector<uint8_t> d0, d1, padded(h * (w + 3), 0xEE);
  EXPECT(ImagePyramid::down(img0.data(), (int)w, (int)h, (int)w, d0, &err));
  for (size_t y = 0; y < h; ++y) std::memcpy(&padded[y * (w + 3)], &img1[y * w], w);
  EXPECT(ImagePyramid::down(padded.data(), (int)w + 3, (int)h, (int)w, d1, &err));
  EXPECT(d0.size() == lh[1] * lw[1] && std::memcmp(d0.data(), want_levels[0].data(), d0.size()) == 0);
  EXPECT(d1.size() == d0.size() && std::memcmp(d1.data(), want_levels[0].data() + d0.size(), d1.size()) == 0);
  // the handle, on a two-image batch in device memory
  malloc_fn dmalloc = reinterpret_cast<malloc_fn>(dlsym(RTLD_DEFAULT, "hipMalloc"));
  free_fn dfree = reinterpret_cast<free_fn>(dlsym(RTLD_DEFAULT, "hipFree"));
  memcpy_fn dcopy = reinterpret_cast<memcpy_fn>(dlsym(RTLD_DEFAULT, "hipMemcpy"));
  EXPECT(dmalloc && dfree && dcopy);
  if (!dmalloc || !dfree || !dcopy) return g_fail;
  ImagePyramid pyr;
  EXPECT(pyr.create((int)h, (int)w, levels, 2) && pyr.valid());
  void* dev = nullptr;
  EXPECT(dmalloc(&dev, 2 * h * w) == 0 && dev);
  if (!dev) return g_fail;
  EXPECT(dcopy(dev, img0.data(), h * w, 1) == 0 && dcopy(static_cast<uint8_t*>(dev) + h * w, img1.data(), h * w, 1) == 0);   // 1: host to device
  EXPECT(!pyr.build(static_cast<const uint8_t*>(dev), (long long)(h * w), (int)w, 3) && has(pyr.error(), "images"));
  EXPECT(pyr.build(static_cast<const uint8_t*>(dev), (long long)(h * w), (int)w, 2));
  for (int l = 0; l < levels; ++l) {
    ImagePyramid::Level L;
    std::vector<uint8_t> got;
    int gh = 0, gw = 0;
    EXPECT(pyr.level(l, &L) && L.h == (int)lh[l] && L.w == (int)lw[l] && L.images == 2 && L.stride >= L.w && L.data);
    EXPECT(l > 0 || (L.data == dev && L.stride == (int)w && L.image_stride == (long long)(h * w)));
    EXPECT(l == 0 || (L.stride % 64 == 0 && L.image_stride == (long long)L.stride * L.h));
    EXPECT(pyr.read_level(l, 0, 2, got, &gh, &gw) && gh == (int)lh[l] && gw == (int)lw[l]);
    if (l == 0) EXPECT(got.size() == 2 * h * w && std::memcmp(got.data(), img0.data(), h * w) == 0 && std::memcmp(got.data() + h * w, img1.data(), h * w) == 0);
    else EXPECT(got == want_levels[l - 1]);
    EXPECT(pyr.read_level(l, 1, 1, got) && got.size() == lh[l] * lw[l]);
    EXPECT(!pyr.read_level(l, 1, 2, got) && has(pyr.error(), "first and count"));
  }
  ImagePyramid::Level L;
  EXPECT(!pyr.level(levels, &L) && has(pyr.error(), "level"));
  float ms = -1.f;
  EXPECT(pyr.bench(2, &ms) && ms >= 0.f);
  pyr.release();
  EXPECT(dfree(dev) == 0);
  // the tracker from host arrays
  PyramidTrackParams p;
  p.levels = levels; p.coarse_radius = hdr[4];
  p.fine.half_window = hdr[5]; p.fine.search_radius = hdr[6]; p.fine.uniqueness = hdr[7]; p.fine.fb_check = hdr[8];
  p.fine.min_texture = fl[0]; p.fine.max_rms = fl[1];
  EXPECT(track_patches_pyramid(img0.data(), (int)w, img1.data(), (int)w, (int)h, (int)w, kp, 3, pred, 3, p, got_kp, got_m0, &got_status, &got_cost, &got_lv, &err));
  EXPECT(got_kp.size() == n * 3 && std::memcmp(got_kp.data(), want_kp.data(), n * 12) == 0);
  EXPECT(got_m0 == want_m0 && got_status == want_status && got_cost == want_cost && got_lv == want_lv);
  int tracked = 0;
  for (uint8_t s : got_status) tracked += s == SSHIP_TRACK_STATUS_TRACKED;
  EXPECT(tracked > 0);
  std::vector<float> k2;
  std::vector<int32_t> m2;
  EXPECT(track_patches_pyramid(img0.data(), (int)w, padded.data(), (int)w + 3, (int)h, (int)w, kp, 3, pred, 3, p, k2, m2, nullptr, nullptr, nullptr, &err));
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
