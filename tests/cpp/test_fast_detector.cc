// The C++ host layer's FAST detector (include/superslam_hip/fast_detector.hpp: superslam_hip::FastParams, FastDetector).
//   no arguments : CPU - the class's and the C ABI's argument validation (false, an error text, nothing thrown; refused before any device)
//   gpu <file>   : GPU - a file the Python test wrote: one image, a keep list and the restatement's outputs.  FastDetector::detect_host
//                  (packed rows and padded ones) and a FastDetector handle on the image in device memory (obtained from the HIP runtime
//                  the library already loaded) give the restatement's bits.
//                  File: i32 {h, w, max_keypoints, n_keep, threshold, border, min_distance, target, n_out, n_candidates}, image [h, w] u8,
//                  keep [max_keypoints, 3] f32, expected kp [max_keypoints, 3] f32, expected carry0 [max_keypoints] i32.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "superslam_hip/fast_detector.hpp"
using namespace superslam_hip;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static constexpr int H = 24, W = 48, MK = 64;

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

static int run_cpu() {
  std::vector<uint8_t> img(H * W, 9);
  std::vector<float> kp, keep(MK * 3, 1.f);
  std::string err;
  auto host = [&](int stride, int h, int w, int mk, const FastParams& p, const uint8_t* im, const float* k = nullptr, int nk = 0) {
    err.clear();
    return FastDetector::detect_host(im, stride, h, w, mk, p, k, nk, kp, nullptr, nullptr, &err);
  };
  FastParams d, p;
  EXPECT(!host(W, 6, W, MK, d, img.data()) && has(err, "h and w"));
  EXPECT(!host(W, H, 16385, MK, d, img.data()) && has(err, "h and w"));
  EXPECT(!host(W, H, W, 0, d, img.data()) && has(err, "max_keypoints"));
  EXPECT(!host(W, H, W, 4097, d, img.data()) && has(err, "max_keypoints"));
  EXPECT(!host(W - 1, H, W, MK, d, img.data()) && has(err, "stride"));
  EXPECT(!host(W, H, W, MK, d, nullptr) && has(err, "null"));
  p = d; p.threshold = 255;
  EXPECT(!host(W, H, W, MK, p, img.data()) && has(err, "threshold"));
  p = d; p.threshold = -1;
  EXPECT(!host(W, H, W, MK, p, img.data()) && has(err, "threshold"));
  p = d; p.border = 2;
  EXPECT(!host(W, H, W, MK, p, img.data()) && has(err, "border"));
  p = d; p.border = 65;
  EXPECT(!host(W, H, W, MK, p, img.data()) && has(err, "border"));
  p = d; p.min_distance = 33;
  EXPECT(!host(W, H, W, MK, p, img.data()) && has(err, "min_distance"));
  p = d; p.selection = 2;
  EXPECT(!host(W, H, W, MK, p, img.data()) && has(err, "selection"));
  p = d; p.selection = SSHIP_SELECT_BALANCED; p.bucket_px = 7;
  EXPECT(!host(W, H, W, MK, p, img.data()) && has(err, "bucket_px"));
  p = d; p.max_new = MK + 1;
  EXPECT(!host(W, H, W, MK, p, img.data()) && has(err, "max_new"));
  p = d; p.target = -1;
  EXPECT(!host(W, H, W, MK, p, img.data()) && has(err, "target"));
  EXPECT(!host(W, H, W, MK, d, img.data(), keep.data(), MK + 1) && has(err, "n_keep"));
  EXPECT(!host(W, H, W, MK, d, img.data(), keep.data(), -1) && has(err, "n_keep"));
  EXPECT(kp.empty());   // a failed call leaves the output alone
  FastDetector f;
  EXPECT(!f.valid());
  EXPECT(!f.create(6, W) && has(f.error(), "h and w") && !f.create(H, W, 0) && has(f.error(), "max_keypoints"));
  EXPECT(!f.create(H, W, MK, 0) && has(f.error(), "max_images") && !f.create(H, W, MK, 65536) && has(f.error(), "max_images") && !f.valid());
  float ms = 0.f;
  int n = 0;
  EXPECT(!f.detect(img.data(), 0, W, 1, nullptr, nullptr, 1, keep.data(), &n) && has(f.error(), "null") && !f.set_params(d) && !f.params(&p) &&
         !f.bench(1, &ms));
  EXPECT(sship_fast_create(H, W, MK, 1, nullptr) == SSHIP_ERR_INVALID && has(sship_last_error(), "null"));
  EXPECT(sship_fast_score_batch_device(nullptr, 0, W, 1, H, W, img.data(), 0, W, nullptr) == SSHIP_ERR_INVALID && has(sship_last_error(), "null"));
  EXPECT(sship_fast_score_batch_device(img.data(), 0, W - 1, 1, H, W, img.data(), 0, W, nullptr) == SSHIP_ERR_INVALID && has(sship_last_error(), "stride"));
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
  int32_t hdr[10];
  std::vector<uint8_t> img;
  std::vector<float> keep, want_kp;
  std::vector<int32_t> want_carry;
  bool ok = std::fread(hdr, 4, 10, f) == 10;
  const size_t h = ok ? hdr[0] : 0, w = ok ? hdr[1] : 0, mk = ok ? hdr[2] : 0;
  const int n_keep = ok ? hdr[3] : 0, n_out = ok ? hdr[8] : 0, n_cand = ok ? hdr[9] : 0;
  ok = ok && read_n(f, img, h * w) && read_n(f, keep, mk * 3) && read_n(f, want_kp, mk * 3) && read_n(f, want_carry, mk);
  std::fclose(f);
  EXPECT(ok);
  if (!ok) return g_fail;
  FastParams p;
  p.threshold = hdr[4]; p.border = hdr[5]; p.min_distance = hdr[6]; p.target = hdr[7];
  std::string err;
  // one image from host arrays, packed and with padded rows
  std::vector<float> k0, k1;
  std::vector<int32_t> c0;
  std::vector<uint8_t> padded(h * (w + 3), 0xEE);
  int cand = -1;
  EXPECT(FastDetector::detect_host(img.data(), (int)w, (int)h, (int)w, (int)mk, p, keep.data(), n_keep, k0, &c0, &cand, &err));
  for (size_t y = 0; y < h; ++y) std::memcpy(&padded[y * (w + 3)], &img[y * w], w);
  EXPECT(FastDetector::detect_host(padded.data(), (int)w + 3, (int)h, (int)w, (int)mk, p, keep.data(), n_keep, k1, nullptr, nullptr, &err));
  EXPECT(cand == n_cand && k0.size() == (size_t)n_out * 3 && std::memcmp(k0.data(), want_kp.data(), k0.size() * 4) == 0 && k1.size() == k0.size() &&
         std::memcmp(k1.data(), k0.data(), k0.size() * 4) == 0);
  EXPECT(c0.size() == (size_t)n_keep && std::memcmp(c0.data(), want_carry.data(), c0.size() * 4) == 0);
  // the handle, on the image in device memory
  malloc_fn dmalloc = reinterpret_cast<malloc_fn>(dlsym(RTLD_DEFAULT, "hipMalloc"));
  free_fn dfree = reinterpret_cast<free_fn>(dlsym(RTLD_DEFAULT, "hipFree"));
  memcpy_fn dcopy = reinterpret_cast<memcpy_fn>(dlsym(RTLD_DEFAULT, "hipMemcpy"));
  sync_fn dsync = reinterpret_cast<sync_fn>(dlsym(RTLD_DEFAULT, "hipDeviceSynchronize"));
  EXPECT(dmalloc && dfree && dcopy && dsync);
  if (!dmalloc || !dfree || !dcopy || !dsync) return g_fail;
  FastDetector d;
  EXPECT(d.create((int)h, (int)w, (int)mk, 1, p) && d.valid());
  FastParams q;
  FastDetector::Shape s;
  EXPECT(d.params(&q, &s) && s.h == (int)h && s.w == (int)w && s.max_keypoints == (int)mk && s.max_images == 1 && q.threshold == p.threshold &&
         q.border == p.border && q.min_distance == p.min_distance && q.target == p.target && q.max_new == (int)mk);
  void *src = nullptr, *dkeep = nullptr, *dout = nullptr, *dints = nullptr;
  EXPECT(dmalloc(&src, h * w) == 0 && dmalloc(&dkeep, mk * 12) == 0 && dmalloc(&dout, mk * 12) == 0 && dmalloc(&dints, (mk + 3) * 4) == 0);
  if (!src || !dkeep || !dout || !dints) return g_fail;
  int32_t* ints = static_cast<int32_t*>(dints);   // n_keep | n_out | n_candidates | carry0 [mk]
  const int32_t nk = n_keep;
  EXPECT(dcopy(src, img.data(), h * w, 1) == 0 && dcopy(dkeep, keep.data(), mk * 12, 1) == 0 && dcopy(ints, &nk, 4, 1) == 0);   // 1: host to device
  float ms = -1.f;
  EXPECT(!d.bench(2, &ms) && has(d.error(), "detect"));
  EXPECT(!d.detect(static_cast<const uint8_t*>(src), 0, (int)w, 2, nullptr, nullptr, 1, static_cast<float*>(dout), ints + 1) && has(d.error(), "images"));
  EXPECT(!d.detect(static_cast<const uint8_t*>(src), 0, (int)w, 1, static_cast<const float*>(dkeep), ints, 1, static_cast<float*>(dkeep), ints + 1) &&
         has(d.error(), "overlap"));
  EXPECT(d.detect(static_cast<const uint8_t*>(src), 0, (int)w, 1, static_cast<const float*>(dkeep), ints, 1, static_cast<float*>(dout), ints + 1, ints + 3,
                  ints + 2));
  std::vector<float> got(mk * 3);
  std::vector<int32_t> gi(mk + 3);
  EXPECT(dsync() == 0 && dcopy(got.data(), dout, mk * 12, 2) == 0 && dcopy(gi.data(), ints, (mk + 3) * 4, 2) == 0);   // 2: device to host
  EXPECT(gi[1] == n_out && gi[2] == n_cand && std::memcmp(got.data(), want_kp.data(), mk * 12) == 0 &&
         std::memcmp(gi.data() + 3, want_carry.data(), mk * 4) == 0);
  EXPECT(d.bench(2, &ms) && ms >= 0.f);
  d.release();
  EXPECT(dfree(src) == 0 && dfree(dkeep) == 0 && dfree(dout) == 0 && dfree(dints) == 0);
  return g_fail;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 2 && std::strcmp(argv[1], "gpu") == 0;
  const int rc = gpu ? run_gpu(argv[2]) : run_cpu();
  if (rc) { std::printf("%d check(s) failed\n", rc); return 1; }
  std::printf("all checks passed (%s)\n", gpu ? "gpu" : "cpu");
  return 0;
}
