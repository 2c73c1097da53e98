// superslam_hip/rectifier.hpp - the image stage in front of the extractor (include/sship.h "Rectification", "RGB-D association"):
//   superslam_hip::Rectifier      the reference's EuRoC runner builds four tables with cv::initUndistortRectifyMap and calls cv::remap on
//                                 both images of every frame (examples/stereo/euroc.cc:88-133,176-177); this class holds the tables on the
//                                 device and remaps a host image (remap: the drop-in for one cv::remap call) or a device batch.
//   superslam_hip::rgbd_associate the per-keypoint loop of RgbdFrontEnd::process (src/RgbdFrontEnd.cc:27-56) for one frame from host arrays.
// Images are (const uint8_t*, row stride) where the reference has a cv::Mat.  A failed call returns false, never throws, and records
// last_error().  The handle is created by the first set_camera / set_maps.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../sship.h"

namespace superslam_hip {

class Rectifier {
public:
  Rectifier(int src_w, int src_h, int dst_w, int dst_h, int cameras = 2)
      : src_w_(src_w), src_h_(src_h), dst_w_(dst_w), dst_h_(dst_h), cameras_(cameras) {}
  ~Rectifier() { if (rect_) sship_rect_destroy(rect_); }
  Rectifier(const Rectifier&) = delete;
  Rectifier& operator=(const Rectifier&) = delete;

  // cv::initUndistortRectifyMap(K, D, R, Pnew, size, CV_32F) without a device: tables are [dst_h * dst_w]
  static bool build_maps(const double K[9], const double* D, int n_dist, const double* R, const double Pnew[9], int dst_w, int dst_h,
                         std::vector<float>& map_x, std::vector<float>& map_y, std::string* error = nullptr) {
    if (dst_w < 1 || dst_h < 1 || dst_w > 4096 || dst_h > 4096) { if (error) *error = "Rectifier::build_maps: dst_w and dst_h must be in [1, 4096]"; return false; }
    map_x.resize(static_cast<size_t>(dst_w) * dst_h);
    map_y.resize(static_cast<size_t>(dst_w) * dst_h);
    if (sship_rect_build_maps(K, D, n_dist, R, Pnew, dst_w, dst_h, map_x.data(), map_y.data()) != SSHIP_OK) {
      if (error) *error = sship_last_error();
      return false;
    }
    return true;
  }
  // K 3x3, D n_dist coefficients (k1 k2 p1 p2 k3 k4 k5 k6; n_dist in {0, 4, 5, 8}), R 3x3 or nullptr, Pnew 3x3 (the left block of P)
  bool set_camera(int camera, const double K[9], const double* D, int n_dist, const double* R, const double Pnew[9]) {
    if (!check_camera(camera, "set_camera") || !ensure()) return false;
    return done(sship_rect_set_camera(rect_, camera, K, D, n_dist, R, Pnew));
  }
  // host fp32 tables [dst_h * dst_w], e.g. the data of the CV_32F maps the caller already holds
  bool set_maps(int camera, const float* map_x, const float* map_y) {
    if (!map_x || !map_y) { last_error_ = "Rectifier::set_maps: null table"; return false; }
    if (!check_camera(camera, "set_maps") || !ensure()) return false;
    return done(sship_rect_set_maps(rect_, camera, map_x, map_y));
  }
  // one host image [src_h, src_stride] -> dst [dst_h, dst_w] contiguous: cv::remap(src, dst, map_x, map_y, INTER_LINEAR)
  bool remap(int camera, const uint8_t* src, int src_stride, uint8_t* dst) {
    if (!src || !dst) { last_error_ = "Rectifier::remap: null image"; return false; }
    if (!check_camera(camera, "remap")) return false;
    if (!rect_) { last_error_ = "Rectifier::remap: no maps set"; return false; }
    return done(sship_rect_remap_host(rect_, camera, src, src_stride, dst));
  }
  // src_dev [images, src_h, src_stride] -> dst_dev [images, dst_h, dst_w]; image i uses camera i % cameras; asynchronous on `stream`
  bool remap_batch_device(const uint8_t* src_dev, int images, int src_stride, uint8_t* dst_dev, void* stream = nullptr) {
    if (!src_dev || !dst_dev) { last_error_ = "Rectifier::remap_batch_device: null image"; return false; }
    if (!rect_) { last_error_ = "Rectifier::remap_batch_device: no maps set"; return false; }
    return done(sship_rect_remap_batch_device(rect_, src_dev, images, src_stride, dst_dev, stream));
  }
  int cameras() const { return cameras_; }
  const std::string& last_error() const { return last_error_; }
  sship_rect* handle() const { return rect_; }

private:
  bool check_camera(int camera, const char* who) {
    if (camera >= 0 && camera < cameras_) return true;
    last_error_ = std::string("Rectifier::") + who + ": camera must be in [0, cameras)";
    return false;
  }
  bool ensure() {
    if (rect_) return true;
    if (sship_rect_create(src_w_, src_h_, dst_w_, dst_h_, cameras_, &rect_) == SSHIP_OK) return true;
    last_error_ = sship_last_error();
    rect_ = nullptr;
    return false;
  }
  bool done(int rc) {
    if (rc == SSHIP_OK) return true;
    last_error_ = sship_last_error();
    return false;
  }
  int src_w_, src_h_, dst_w_, dst_h_, cameras_;
  sship_rect* rect_ = nullptr;
  std::string last_error_;
};

// One frame of RgbdFrontEnd::process from host arrays: keypoints [n] x (x, y) with `kp_stride` floats between them, depth [h, depth_stride
// bytes] u16 or f32.  Outputs (each n entries): undistorted (u', v') pairs, stereo triples (u', uR or NaN, v'), has_depth bytes.
inline bool rgbd_associate(const float* keypoints, int kp_stride, int n, const void* depth, int depth_type, int h, int w, int depth_stride,
                           const sship_rgbd_params& params, std::vector<float>& undistorted, std::vector<float>& stereo,
                           std::vector<uint8_t>& has_depth, std::string* error = nullptr) {
  undistorted.assign(n > 0 ? static_cast<size_t>(n) * 2 : 0, 0.f);
  stereo.assign(n > 0 ? static_cast<size_t>(n) * 3 : 0, 0.f);
  has_depth.assign(n > 0 ? static_cast<size_t>(n) : 0, 0);
  if (sship_rgbd_associate_host(keypoints, kp_stride, n, depth, depth_type, h, w, depth_stride, &params, undistorted.data(), stereo.data(),
                                has_depth.data()) == SSHIP_OK)
    return true;
  if (error) *error = sship_last_error();
  undistorted.clear(); stereo.clear(); has_depth.clear();
  return false;
}

}  // namespace superslam_hip
