// superslam_hip/binary_descriptor.hpp - steered BRIEF descriptors and the Hamming matcher on the device (include/sship.h "Binary
// descriptors", "Hamming matcher"):
//   superslam_hip::describe_brief         256-bit descriptors at given keypoints of one host image - where a classical front end would
//                                         call cv::ORB::compute; describe_brief_device is the batch form on device memory
//   superslam_hip::brief_pattern          the rotated test table of an orientation bin (no GPU)
//   superslam_hip::HammingMatcher         the library's sship_hm handle: mutual nearest neighbour under the Hamming distance with an
//                                         optional keypoint-window gate - where the reference would use cv::BFMatcher(NORM_HAMMING)
// Images are (const uint8_t*, row stride); keypoints are (x, y, score) float rows; a descriptor is 8 uint32_t.  A failed call returns
// false, never throws, and reports the library's message through error() / `error`.
#pragma once
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "../sship.h"

namespace superslam_hip {

enum class BriefMode { Steered = SSHIP_BRIEF_STEERED, Upright = SSHIP_BRIEF_UPRIGHT };

// int8 (ax', ay', bx', by') rows of bin 0..31
inline bool brief_pattern(int bin, std::vector<int8_t>& out, std::string* error = nullptr) {
  std::vector<int8_t> t(256 * 4);
  if (sship_brief_pattern(bin, t.data()) != SSHIP_OK) {
    if (error) *error = sship_last_error();
    return false;
  }
  out.swap(t);
  return true;
}

// one host image: img [h, stride bytes], n keypoint rows kp_stride >= 2 floats apart -> desc [n][8], status [n] (SSHIP_BRIEF_*), bin [n]
inline bool describe_brief(const uint8_t* img, int stride, int h, int w, const float* keypoints, int kp_stride, int n, BriefMode mode,
                           std::vector<uint32_t>& desc, std::vector<uint8_t>* status = nullptr, std::vector<uint8_t>* bin = nullptr,
                           std::string* error = nullptr) {
  if (n < 0 || n > 4096) {
    if (error) *error = "describe_brief: n must be in [0, 4096]";
    return false;
  }
  const size_t m = static_cast<size_t>(n);
  std::vector<uint32_t> d(m * 8);
  std::vector<uint8_t> s(m), b(m);
  if (sship_brief_describe_host(img, stride, h, w, keypoints, kp_stride, n, static_cast<int>(mode), d.data(), s.data(), b.data()) != SSHIP_OK) {
    if (error) *error = sship_last_error();
    return false;
  }
  desc.swap(d);
  if (status) status->swap(s);
  if (bin) bin->swap(b);
  return true;
}

// `images` device images, image i at imgs_dev + i * image_stride in rows of `stride` bytes; kp_dev [units, max_keypoints, 3] with counts
// n_dev (image i reads unit i * unit_stride) -> desc_dev [images, max_keypoints, 8], status_dev / bin_dev [images, max_keypoints] or
// nullptr.  Asynchronous on `stream`, one launch.
inline bool describe_brief_device(const uint8_t* imgs_dev, long long image_stride, int stride, int images, int h, int w, const float* kp_dev,
                                  const int* n_dev, int unit_stride, int max_keypoints, BriefMode mode, uint32_t* desc_dev,
                                  uint8_t* status_dev = nullptr, uint8_t* bin_dev = nullptr, void* stream = nullptr, std::string* error = nullptr) {
  if (sship_brief_describe_batch_device(imgs_dev, image_stride, stride, images, h, w, kp_dev, n_dev, unit_stride, max_keypoints,
                                        static_cast<int>(mode), desc_dev, status_dev, bin_dev, stream) == SSHIP_OK)
    return true;
  if (error) *error = sship_last_error();
  return false;
}

struct HammingParams {
  int max_distance = 0;       // [0, 256]; 0: off
  int ratio_percent = 0;      // [0, 100]; 0: off
  bool mutual_check = true;
};

class HammingMatcher {
 public:
  struct Gate { bool enabled = false; float dx_lo = 0, dx_hi = 0, dy_lo = 0, dy_hi = 0; };

  HammingMatcher() = default;
  HammingMatcher(const HammingMatcher&) = delete;
  HammingMatcher& operator=(const HammingMatcher&) = delete;
  ~HammingMatcher() { release(); }

  // max_keypoints in [1, 4096], max_pairs in [1, 65535]; every workspace is allocated here and nothing later
  bool create(int max_keypoints = 1024, int max_pairs = 1, const HammingParams& params = HammingParams()) {
    release();
    if (!ok(sship_hm_create(max_keypoints, max_pairs, &hm_))) return false;
    if (set_params(params)) return true;
    release();
    return false;
  }
  void release() { if (hm_) sship_hm_destroy(hm_); hm_ = nullptr; }
  bool valid() const { return hm_ != nullptr; }
  sship_hm* handle() const { return hm_; }
  const std::string& error() const { return error_; }

  bool set_params(const HammingParams& p) { return ok(sship_hm_set_params(hm_, p.max_distance, p.ratio_percent, p.mutual_check ? 1 : 0)); }
  bool params(HammingParams* out, int* max_keypoints = nullptr, int* max_pairs = nullptr) {
    int d = 0, r = 0, m = 0;
    if (!ok(sship_hm_get_params(hm_, &d, &r, &m, max_keypoints, max_pairs))) return false;
    if (out) { out->max_distance = d; out->ratio_percent = r; out->mutual_check = m != 0; }
    return true;
  }
  // an entry is present only if dx_lo <= x0 - x1 <= dx_hi and dy_lo <= y0 - y1 <= dy_hi (bounds may be infinite)
  bool set_gate(float dx_lo, float dx_hi, float dy_lo, float dy_hi) { return ok(sship_hm_set_gate(hm_, 1, dx_lo, dx_hi, dy_lo, dy_hi)); }
  bool set_stereo_gate(float min_disparity, float max_disparity, float max_row_diff = 2.f) {
    return set_gate(min_disparity, max_disparity, -max_row_diff, max_row_diff);
  }
  bool clear_gate() {
    const float inf = std::numeric_limits<float>::infinity();
    return ok(sship_hm_set_gate(hm_, 0, -inf, inf, -inf, inf));
  }
  bool gate(Gate* g) {
    int on = 0;
    Gate t;
    if (!ok(sship_hm_get_gate(hm_, &on, &t.dx_lo, &t.dx_hi, &t.dy_lo, &t.dy_hi))) return false;
    t.enabled = on != 0;
    if (g) *g = t;
    return true;
  }

  // set 0 of pair p is unit first0 + p * step0, set 1 unit first1 + p * step1 of n_dev [units], desc_dev [units, max_keypoints, 8],
  // status_dev [units, max_keypoints] (or nullptr) and kp_dev [units, max_keypoints, 3] (nullptr unless gated) -> matches0_dev, dist0_dev
  // [pairs, max_keypoints], mscores0_dev the same or nullptr.  Asynchronous on `stream`.
  bool match(const int* n_dev, const uint32_t* desc_dev, const uint8_t* status_dev, const float* kp_dev, int first0, int step0, int first1, int step1,
             int pairs, int32_t* matches0_dev, int32_t* dist0_dev, float* mscores0_dev = nullptr, void* stream = nullptr) {
    return ok(sship_hm_match_batch_device(hm_, n_dev, desc_dev, status_dev, kp_dev, first0, step0, first1, step1, pairs, matches0_dev, dist0_dev,
                                          mscores0_dev, stream));
  }
  // one pair from host arrays: desc [n][8]; status may be nullptr; keypoints (rows of 3 floats) are read only when the gate is on
  bool match_host(int n0, const uint32_t* desc0, const uint8_t* status0, const float* kp0, int n1, const uint32_t* desc1, const uint8_t* status1,
                  const float* kp1, std::vector<int32_t>& matches0, std::vector<int32_t>* dist0 = nullptr, std::vector<float>* mscores0 = nullptr) {
    const size_t m = n0 > 0 ? static_cast<size_t>(n0) : 0;
    std::vector<int32_t> m0(m, -1), d0(m, -1);
    std::vector<float> ms(m, 0.f);
    if (!ok(sship_hm_match_host(hm_, n0, desc0, status0, kp0, 3, n1, desc1, status1, kp1, 3, m0.data(), d0.data(), ms.data()))) return false;
    matches0.swap(m0);
    if (dist0) dist0->swap(d0);
    if (mscores0) mscores0->swap(ms);
    return true;
  }
  bool bench(int iters, float* avg_ms) { return ok(sship_hm_bench(hm_, iters, avg_ms)); }

 private:
  bool ok(int rc) {
    if (rc == SSHIP_OK) return true;
    error_ = sship_last_error();
    return false;
  }
  sship_hm* hm_ = nullptr;
  std::string error_;
};

}  // namespace superslam_hip
