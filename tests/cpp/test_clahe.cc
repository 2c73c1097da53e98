// The C++ host layer's CLAHE (include/superslam_hip/clahe.hpp: superslam_hip::Clahe).
//   no arguments : CPU - the class's and the C ABI's argument validation (false, an error text, nothing thrown; refused before any device)
//   gpu <file>   : GPU - a file the Python test wrote: a batch of images and the restatement's tables and pixels for two clip limits.
//                  Clahe::apply_host (packed rows and padded ones) and a Clahe handle on the batch in device memory (obtained from the HIP
//                  runtime the library already loaded; a destination of its own, then in place after set_clip_limit) give the restatement's
//                  bits.
//                  File: i32 {h, w, tiles_x, tiles_y, n}, f64 {clip0, clip1}, images [n, h, w] u8, then for each clip the expected tables
//                  [n, tiles_y, tiles_x, 256] u8 and the expected output [n, h, w] u8.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "superslam_hip/clahe.hpp"
using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static constexpr int H = 24, W = 48;

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

static int run_cpu() {
  std::vector<uint8_t> img(H * W, 9), out;
  std::string err;
  auto host = [&](int stride, int h, int w, int tx, int ty, double clip, const uint8_t* p) {
    err.clear();
    return Clahe::apply_host(p, stride, h, w, tx, ty, clip, out, &err);
  };
  EXPECT(!host(W, 0, W, 8, 8, 40.0, img.data()) && has(err, "h and w"));
  EXPECT(!host(W, H, 16385, 8, 8, 40.0, img.data()) && has(err, "h and w"));
  EXPECT(!host(W, H, W, 0, 8, 40.0, img.data()) && has(err, "tiles"));
  EXPECT(!host(W, H, W, 8, 17, 40.0, img.data()) && has(err, "tiles"));
  EXPECT(!host(W, H, W, 8, 8, -1.0, img.data()) && has(err, "clip_limit"));
  EXPECT(!host(W, H, W, 8, 8, std::numeric_limits<double>::quiet_NaN(), img.data()) && has(err, "clip_limit"));
  EXPECT(!host(W, H, W, 8, 8, std::numeric_limits<double>::infinity(), img.data()) && has(err, "clip_limit"));
  EXPECT(!host(W - 1, H, W, 8, 8, 40.0, img.data()) && has(err, "stride"));
  EXPECT(!host(W, H, W, 8, 8, 40.0, nullptr) && has(err, "null"));
  EXPECT(!host(8, 3, 8, 8, 2, 40.0, img.data()) && has(err, "extension"));    // w = 8 divides, h = 3 does not: ew - w = 8 > 7
  EXPECT(!host(9, 2, 9, 8, 8, 40.0, img.data()) && has(err, "extension"));    // eh - h = 6 > 1
  EXPECT(!host(4097, 4097, 4097, 1, 1, 40.0, img.data()) && has(err, "2^24"));
  EXPECT(out.empty());   // a failed call leaves the output alone
  Clahe c;
  EXPECT(!c.valid());
  EXPECT(!c.create(0, W) && has(c.error(), "h and w") && !c.create(H, W, 17, 8) && has(c.error(), "tiles"));
  EXPECT(!c.create(H, W, 8, 8, -0.5) && has(c.error(), "clip_limit") && !c.create(H, W, 8, 8, 40.0, 0) && has(c.error(), "max_images"));
  EXPECT(!c.create(H, W, 8, 8, 40.0, 65536) && has(c.error(), "max_images") && !c.create(8, 8, 8, 3) && has(c.error(), "extension") && !c.valid());
  Clahe::Params p;
  float ms = 0.f;
  EXPECT(!c.apply(img.data(), 0, W, img.data(), 0, W, 1) && has(c.error(), "null") && !c.set_clip_limit(3.0) && !c.params(&p) && !c.luts(0, 1, out) &&
         !c.bench(1, &ms));
  EXPECT(sship_clahe_create(H, W, 8, 8, 40.0, 1, nullptr) == SSHIP_ERR_INVALID && has(sship_last_error(), "null"));
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
typedef int (*sync_fn)();

static int run_gpu(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) { std::printf("cannot open %s\n", path); return 1; }
  int32_t hdr[5];
  double clip[2];
  std::vector<uint8_t> imgs, want_luts[2], want_out[2];
  bool ok = std::fread(hdr, 4, 5, f) == 5 && std::fread(clip, 8, 2, f) == 2;
  const size_t h = ok ? hdr[0] : 0, w = ok ? hdr[1] : 0, n = ok ? hdr[4] : 0;
  const int tx = ok ? hdr[2] : 0, ty = ok ? hdr[3] : 0;
  const size_t img = h * w, tab = (size_t)tx * ty * 256;
  ok = ok && read_n(f, imgs, n * img);
  for (int k = 0; k < 2; ++k) ok = ok && read_n(f, want_luts[k], n * tab) && read_n(f, want_out[k], n * img);
  std::fclose(f);
  EXPECT(ok && n >= 2);
  if (!ok || n < 2) return g_fail;
  std::string err;
  // one image from host arrays, packed and with padded rows
  std::vector<uint8_t> d0, d1, padded(h * (w + 3), 0xEE);
  EXPECT(Clahe::apply_host(imgs.data(), (int)w, (int)h, (int)w, tx, ty, clip[0], d0, &err));
  for (size_t y = 0; y < h; ++y) std::memcpy(&padded[y * (w + 3)], &imgs[img + y * w], w);
  EXPECT(Clahe::apply_host(padded.data(), (int)w + 3, (int)h, (int)w, tx, ty, clip[1], d1, &err));
  EXPECT(d0.size() == img && std::memcmp(d0.data(), want_out[0].data(), img) == 0);
  EXPECT(d1.size() == img && std::memcmp(d1.data(), want_out[1].data() + img, img) == 0);
  // the handle, on the batch in device memory
  malloc_fn dmalloc = reinterpret_cast<malloc_fn>(dlsym(RTLD_DEFAULT, "hipMalloc"));
  free_fn dfree = reinterpret_cast<free_fn>(dlsym(RTLD_DEFAULT, "hipFree"));
  memcpy_fn dcopy = reinterpret_cast<memcpy_fn>(dlsym(RTLD_DEFAULT, "hipMemcpy"));
  sync_fn dsync = reinterpret_cast<sync_fn>(dlsym(RTLD_DEFAULT, "hipDeviceSynchronize"));
  EXPECT(dmalloc && dfree && dcopy && dsync);
  if (!dmalloc || !dfree || !dcopy || !dsync) return g_fail;
  Clahe c;
  EXPECT(c.create((int)h, (int)w, tx, ty, clip[0], (int)n) && c.valid());
  Clahe::Params p;
  EXPECT(c.params(&p) && p.h == (int)h && p.w == (int)w && p.tiles_x == tx && p.tiles_y == ty && p.max_images == (int)n && p.clip_limit == clip[0]);
  void *src = nullptr, *dst = nullptr;
  EXPECT(dmalloc(&src, n * img) == 0 && src && dmalloc(&dst, n * img) == 0 && dst);
  if (!src || !dst) return g_fail;
  EXPECT(dcopy(src, imgs.data(), n * img, 1) == 0);   // 1: host to device
  std::vector<uint8_t> got(n * img), luts;
  EXPECT(!c.luts(0, 1, luts) && has(c.error(), "apply"));
  EXPECT(!c.apply(static_cast<const uint8_t*>(src), (long long)img, (int)w, static_cast<uint8_t*>(dst), (long long)img, (int)w, (int)n + 1) &&
         has(c.error(), "images"));
  EXPECT(c.apply(static_cast<const uint8_t*>(src), (long long)img, (int)w, static_cast<uint8_t*>(dst), (long long)img, (int)w, (int)n));
  EXPECT(dsync() == 0 && dcopy(got.data(), dst, n * img, 2) == 0);   // 2: device to host
  EXPECT(got == want_out[0]);
  EXPECT(c.luts(0, (int)n, luts) && luts == want_luts[0]);
  EXPECT(c.luts(1, 1, luts) && luts.size() == tab && std::memcmp(luts.data(), want_luts[0].data() + tab, tab) == 0);
  EXPECT(!c.luts(1, (int)n, luts) && has(c.error(), "first and count"));
  float ms = -1.f;
  EXPECT(c.bench(2, &ms) && ms >= 0.f);
  // another limit, in place
  EXPECT(c.set_clip_limit(clip[1]) && c.params(&p) && p.clip_limit == clip[1]);
  EXPECT(c.apply(static_cast<const uint8_t*>(src), (long long)img, (int)w, static_cast<uint8_t*>(src), (long long)img, (int)w, (int)n));
  EXPECT(dsync() == 0 && dcopy(got.data(), src, n * img, 2) == 0);
  EXPECT(got == want_out[1]);
  EXPECT(c.luts(0, (int)n, luts) && luts == want_luts[1]);
  c.release();
  EXPECT(dfree(src) == 0 && dfree(dst) == 0);
  return g_fail;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 2 && std::strcmp(argv[1], "gpu") == 0;
  const int rc = gpu ? run_gpu(argv[2]) : run_cpu();
  if (rc) { std::printf("%d check(s) failed\n", rc); return 1; }
  std::printf("all checks passed (%s)\n", gpu ? "gpu" : "cpu");
  return 0;
}
