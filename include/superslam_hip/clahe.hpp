// superslam_hip/clahe.hpp - contrast-limited adaptive histogram equalisation on the device (include/sship.h "CLAHE"):
//   superslam_hip::Clahe    the library's sship_clahe handle: a batch of u8 images in device memory equalised with two launches;
//                           Clahe::apply_host is one host image - where the reference pipelines would call cv::CLAHE::apply.
// Images are (const uint8_t*, row stride) where the reference has a cv::Mat.  A failed call returns false, never throws, and reports the
// library's message through error() / `error`.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../sship.h"

namespace superslam_hip {

class Clahe {
 public:
  struct Params { int h = 0, w = 0, tiles_x = 0, tiles_y = 0, max_images = 0; double clip_limit = 0.0; };

  Clahe() = default;
  Clahe(const Clahe&) = delete;
  Clahe& operator=(const Clahe&) = delete;
  ~Clahe() { release(); }

  // h and w in [1, 16384], tiles in [1, 16], clip_limit finite and >= 0 (0: no clipping), max_images in [1, 65535]; the table workspace
  // is allocated here and nothing later
  bool create(int h, int w, int tiles_x = 8, int tiles_y = 8, double clip_limit = 40.0, int max_images = 1) {
    release();
    return ok(sship_clahe_create(h, w, tiles_x, tiles_y, clip_limit, max_images, &clahe_));
  }
  void release() { if (clahe_) sship_clahe_destroy(clahe_); clahe_ = nullptr; }
  bool valid() const { return clahe_ != nullptr; }
  sship_clahe* handle() const { return clahe_; }
  const std::string& error() const { return error_; }

  bool set_clip_limit(double clip_limit) { return ok(sship_clahe_set_clip_limit(clahe_, clip_limit)); }
  bool params(Params* out) {
    Params p;
    if (!out || !ok(sship_clahe_get_params(clahe_, &p.h, &p.w, &p.tiles_x, &p.tiles_y, &p.clip_limit, &p.max_images))) return false;
    *out = p;
    return true;
  }

  // `images` device images of h x w bytes: image i is read at src_dev + i * src_image_stride in rows of src_stride bytes and written at
  // dst_dev + i * dst_image_stride in rows of dst_stride bytes.  dst_dev == src_dev with equal strides: in place.  Asynchronous on `stream`.
  bool apply(const uint8_t* src_dev, long long src_image_stride, int src_stride, uint8_t* dst_dev, long long dst_image_stride, int dst_stride,
             int images, void* stream = nullptr) {
    return ok(sship_clahe_apply_batch_device(clahe_, src_dev, src_image_stride, src_stride, dst_dev, dst_image_stride, dst_stride, images, stream));
  }
  // the tables of images [first, first + count) of the last call, packed: count x tiles_y x tiles_x x 256 bytes.  Synchronous.
  bool luts(int first, int count, std::vector<uint8_t>& out) {
    Params p;
    if (!params(&p)) return false;
    if (count < 1) { error_ = "luts: count must be >= 1"; return false; }
    std::vector<uint8_t> buf(static_cast<size_t>(count) * p.tiles_x * p.tiles_y * 256);
    if (!ok(sship_clahe_read_luts(clahe_, first, count, buf.data()))) return false;
    out.swap(buf);
    return true;
  }
  bool bench(int iters, float* avg_ms) { return ok(sship_clahe_bench(clahe_, iters, avg_ms)); }

  // one host image: src [h, stride bytes] -> dst, packed h x w bytes
  static bool apply_host(const uint8_t* src, int stride, int h, int w, int tiles_x, int tiles_y, double clip_limit, std::vector<uint8_t>& dst,
                         std::string* error = nullptr) {
    if (h < 1 || w < 1 || h > 16384 || w > 16384) {
      if (error) *error = "Clahe::apply_host: h and w must be in [1, 16384]";
      return false;
    }
    std::vector<uint8_t> buf(static_cast<size_t>(h) * w);
    if (sship_clahe_apply_host(src, stride, h, w, tiles_x, tiles_y, clip_limit, buf.data(), w) != SSHIP_OK) {
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
  sship_clahe* clahe_ = nullptr;
  std::string error_;
};

}  // namespace superslam_hip
