// superslam_hip/fast_detector.hpp - FAST corners with track refill on the device (include/sship.h "FAST corners"):
//   superslam_hip::FastParams    the rule's parameters (sship_fast_params with its defaults)
//   superslam_hip::FastDetector  the library's sship_fast handle: corners of a batch of u8 images in device memory, merged behind the live
//                                rows of a keypoint list; FastDetector::detect_host is one host image - where a classical front end
//                                would call cv::FAST and cv::goodFeaturesToTrack's mask.
// Images are (const uint8_t*, row stride) where the reference has a cv::Mat; keypoints are (x, y, score) float rows.  A failed call
// returns false, never throws, and reports the library's message through error() / `error`.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../sship.h"

namespace superslam_hip {

struct FastParams {
  int threshold = 20;                  // t in [0, 254]: a corner has s > t
  int border = 8;                      // b in [3, 64]
  int min_distance = 10;               // d in [0, 32]: no new corner within d (Chebyshev) of a live row; 0: no mask
  int selection = SSHIP_SELECT_TOPK;   // or SSHIP_SELECT_BALANCED with bucket_px in [8, 65535]
  int bucket_px = 32;
  int max_new = 0;                     // [1, max_keypoints]; 0 here: max_keypoints
  int target = 0;                      // > 0: append only up to `target` rows in all
  sship_fast_params c(int max_keypoints) const {
    return sship_fast_params{threshold, border, min_distance, selection, bucket_px, max_new > 0 ? max_new : max_keypoints, target};
  }
};

class FastDetector {
 public:
  struct Shape { int h = 0, w = 0, max_keypoints = 0, max_images = 0; };

  FastDetector() = default;
  FastDetector(const FastDetector&) = delete;
  FastDetector& operator=(const FastDetector&) = delete;
  ~FastDetector() { release(); }

  // h and w in [7, 16384], max_keypoints in [1, 4096], max_images in [1, 65535]; every workspace is allocated here and nothing later
  bool create(int h, int w, int max_keypoints = 1024, int max_images = 2, const FastParams& params = FastParams()) {
    release();
    if (!ok(sship_fast_create(h, w, max_keypoints, max_images, &fast_))) return false;
    max_keypoints_ = max_keypoints;
    if (set_params(params)) return true;
    release();
    return false;
  }
  void release() { if (fast_) sship_fast_destroy(fast_); fast_ = nullptr; }
  bool valid() const { return fast_ != nullptr; }
  sship_fast* handle() const { return fast_; }
  const std::string& error() const { return error_; }

  bool set_params(const FastParams& params) {
    const sship_fast_params p = params.c(max_keypoints_);
    return ok(sship_fast_set_params(fast_, &p));
  }
  bool params(FastParams* out, Shape* shape = nullptr) {
    sship_fast_params p;
    Shape s;
    if (!ok(sship_fast_get_params(fast_, &p, &s.h, &s.w, &s.max_keypoints, &s.max_images))) return false;
    if (out) { out->threshold = p.threshold; out->border = p.border; out->min_distance = p.min_distance; out->selection = p.selection;
               out->bucket_px = p.bucket_px; out->max_new = p.max_new; out->target = p.target; }
    if (shape) *shape = s;
    return true;
  }

  // `images` device images of h x w bytes, image i at imgs_dev + i * image_stride in rows of `stride` bytes.  keep_dev [units, max_keypoints,
  // 3] with counts keep_n_dev (image i reads unit i * unit_stride) or nullptr; kp_out_dev [images, max_keypoints, 3], n_out_dev [images],
  // carry0_dev [images, max_keypoints] or nullptr, n_candidates_dev [images] or nullptr.  Asynchronous on `stream`.
  bool detect(const uint8_t* imgs_dev, long long image_stride, int stride, int images, const float* keep_dev, const int* keep_n_dev, int unit_stride,
              float* kp_out_dev, int* n_out_dev, int32_t* carry0_dev = nullptr, int* n_candidates_dev = nullptr, void* stream = nullptr) {
    return ok(sship_fast_detect_batch_device(fast_, imgs_dev, image_stride, stride, images, keep_dev, keep_n_dev, unit_stride, kp_out_dev, n_out_dev,
                                             carry0_dev, n_candidates_dev, stream));
  }
  bool bench(int iters, float* avg_ms) { return ok(sship_fast_bench(fast_, iters, avg_ms)); }

  // one host image: img [h, stride bytes]; keep: n_keep rows of (x, y, score) or nullptr -> keypoints [n_out][3] (the live rows first),
  // carry0 [n_keep] (the output row of each keep row or -1), the number of candidates
  static bool detect_host(const uint8_t* img, int stride, int h, int w, int max_keypoints, const FastParams& params, const float* keep, int n_keep,
                          std::vector<float>& keypoints, std::vector<int32_t>* carry0 = nullptr, int* n_candidates = nullptr,
                          std::string* error = nullptr) {
    if (max_keypoints < 1 || max_keypoints > 4096) {
      if (error) *error = "FastDetector::detect_host: max_keypoints must be in [1, 4096]";
      return false;
    }
    const sship_fast_params p = params.c(max_keypoints);
    std::vector<float> kp(static_cast<size_t>(max_keypoints) * 3);
    std::vector<int32_t> carry(static_cast<size_t>(max_keypoints));
    int n_out = 0, n_cand = 0;
    if (sship_fast_detect_host(img, stride, h, w, max_keypoints, &p, keep, 3, n_keep, kp.data(), &n_out, carry.data(), &n_cand) != SSHIP_OK) {
      if (error) *error = sship_last_error();
      return false;
    }
    kp.resize(static_cast<size_t>(n_out) * 3);
    keypoints.swap(kp);
    if (carry0) { carry.resize(keep ? static_cast<size_t>(n_keep) : 0); carry0->swap(carry); }
    if (n_candidates) *n_candidates = n_cand;
    return true;
  }

 private:
  bool ok(int rc) {
    if (rc == SSHIP_OK) return true;
    error_ = sship_last_error();
    return false;
  }
  sship_fast* fast_ = nullptr;
  int max_keypoints_ = 0;
  std::string error_;
};

}  // namespace superslam_hip
