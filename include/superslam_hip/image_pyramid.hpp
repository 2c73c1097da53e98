// superslam_hip/image_pyramid.hpp - a device image pyramid and coarse-to-fine patch tracking on it
// (include/sship.h "Image pyramid" and "Coarse-to-fine patch tracking"):
//   superslam_hip::ImagePyramid          the library's sship_pyr handle: levels 1 and above of a batch of u8 images, built on the device from
//                                        the caller's level 0; ImagePyramid::down is one reduction of one host image - where the reference
//                                        would call cv::pyrDown.
//   superslam_hip::PyramidTrackParams    the library's sship_pyr_track_params with its defaults
//   superslam_hip::track_patches_pyramid one pair from host arrays, as track_patches, with the search walked down `levels` levels
// Images are (const uint8_t*, row stride) where the reference has a cv::Mat.  A failed call returns false, never throws, and reports the
// library's message through error() / `error`.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../sship.h"
#include "patch_tracker.hpp"

namespace superslam_hip {

class ImagePyramid {
 public:
  struct Level { const uint8_t* data = nullptr; int h = 0, w = 0, stride = 0; long long image_stride = 0; int images = 0; };   // device memory

  ImagePyramid() = default;
  ImagePyramid(const ImagePyramid&) = delete;
  ImagePyramid& operator=(const ImagePyramid&) = delete;
  ~ImagePyramid() { release(); }

  // levels 1 .. 8 (level 0 counted), h and w in [1, 16384], max_images in [1, 65535]; everything the handle will ever need is allocated here
  bool create(int h, int w, int levels, int max_images) {
    release();
    return ok(sship_pyr_create(h, w, levels, max_images, &pyr_));
  }
  void release() { if (pyr_) sship_pyr_destroy(pyr_); pyr_ = nullptr; }
  bool valid() const { return pyr_ != nullptr; }
  sship_pyr* handle() const { return pyr_; }
  const std::string& error() const { return error_; }

  // imgs_dev: `images` device images of h x w bytes, image i at imgs_dev + i * image_stride, rows of `stride` bytes; borrowed as level 0 until the
  // next build or release.  Asynchronous on `stream`.
  bool build(const uint8_t* imgs_dev, long long image_stride, int stride, int images, void* stream = nullptr) {
    return ok(sship_pyr_build_batch_device(pyr_, imgs_dev, image_stride, stride, images, stream));
  }
  bool level(int l, Level* out) {
    Level v;
    if (!out || !ok(sship_pyr_level(pyr_, l, &v.data, &v.h, &v.w, &v.stride, &v.image_stride, &v.images))) return false;
    *out = v;
    return true;
  }
  // images [first, first + count) of level l, packed: count x h_l x w_l bytes.  Synchronous.
  bool read_level(int l, int first, int count, std::vector<uint8_t>& out, int* h = nullptr, int* w = nullptr) {
    Level v;
    if (!level(l, &v)) return false;
    if (count < 1) { error_ = "read_level: count must be >= 1"; return false; }
    std::vector<uint8_t> buf(static_cast<size_t>(count) * v.h * v.w);
    if (!ok(sship_pyr_read_level(pyr_, l, first, count, buf.data(), v.w))) return false;
    out.swap(buf);
    if (h) *h = v.h;
    if (w) *w = v.w;
    return true;
  }
  bool bench(int iters, float* avg_ms) { return ok(sship_pyr_bench(pyr_, iters, avg_ms)); }

  // one reduction of one host image: src [h, stride bytes] -> dst, packed ((h + 1) / 2) x ((w + 1) / 2) bytes
  static bool down(const uint8_t* src, int stride, int h, int w, std::vector<uint8_t>& dst, std::string* error = nullptr) {
    if (h < 1 || w < 1 || h > 16384 || w > 16384) {
      if (error) *error = "ImagePyramid::down: h and w must be in [1, 16384]";
      return false;
    }
    std::vector<uint8_t> buf(static_cast<size_t>((h + 1) / 2) * ((w + 1) / 2));
    if (sship_pyr_down_host(src, stride, h, w, buf.data(), (w + 1) / 2) != SSHIP_OK) {
      if (error) *error = sship_last_error();
      return false;
    }
    dst.swap(buf);
    return true;
  }

 private:
  bool ok(int rc) {
    if (rc == SSHIP_OK) return true;
    error_ = sship_last_error();
    return false;
  }
  sship_pyr* pyr_ = nullptr;
  std::string error_;
};

struct PyramidTrackParams {
  PatchTrackParams fine;   // level 0; half_window and uniqueness also hold on the levels above
  int levels = 3;          // levels walked, level 0 counted; 1 .. 8
  int coarse_radius = 8;   // search radius of the levels above 0; 1 .. 16
  sship_pyr_track_params c() const { return sship_pyr_track_params{fine.c(), levels, coarse_radius}; }
};

// arguments as track_patches; levels_tracked (optional) receives per keypoint the bit mask of the levels that ended TRACKED
inline bool track_patches_pyramid(const uint8_t* img0, int stride0, const uint8_t* img1, int stride1, int h, int w, const std::vector<float>& keypoints,
                                  int kp_stride, const std::vector<float>& pred, int pred_stride, const PyramidTrackParams& params,
                                  std::vector<float>& kp_out, std::vector<int32_t>& matches0, std::vector<uint8_t>* status = nullptr,
                                  std::vector<int64_t>* cost = nullptr, std::vector<uint8_t>* levels_tracked = nullptr, std::string* error = nullptr) {
  if (kp_stride < 2 || keypoints.size() % static_cast<size_t>(kp_stride) != 0 || keypoints.size() / static_cast<size_t>(kp_stride) > 4096) {
    if (error) *error = "track_patches_pyramid: keypoints must hold kp_stride >= 2 floats per keypoint, at most 4096 of them";
    return false;
  }
  const size_t n = keypoints.size() / static_cast<size_t>(kp_stride);
  if (!pred.empty() && (pred_stride < 2 || pred.size() != n * static_cast<size_t>(pred_stride))) {
    if (error) *error = "track_patches_pyramid: pred must be empty or hold pred_stride >= 2 floats per keypoint";
    return false;
  }
  std::vector<float> ko(n * 3);
  std::vector<int32_t> mo(n);
  std::vector<uint8_t> st(n), lv(n);
  std::vector<int64_t> co(n);
  const sship_pyr_track_params p = params.c();
  if (sship_patch_track_pyramid_host(img0, stride0, img1, stride1, h, w, keypoints.data(), kp_stride, pred.empty() ? nullptr : pred.data(), pred_stride,
                                     static_cast<int>(n), &p, ko.data(), mo.data(), st.data(), co.data(), lv.data()) != SSHIP_OK) {
    if (error) *error = sship_last_error();
    return false;
  }
  kp_out.swap(ko);
  matches0.swap(mo);
  if (status) status->swap(st);
  if (cost) cost->swap(co);
  if (levels_tracked) levels_tracked->swap(lv);
  return true;
}

}  // namespace superslam_hip
