// superslam_hip/stereo_search.hpp - uR for left keypoints by a patch search along their row of the rectified right image
// (include/sship.h "Stereo search"):
//   superslam_hip::StereoSearchParams  the library's sship_stereo_search_params with its defaults
//   superslam_hip::search_stereo       one pair from host arrays: the left keypoints in, the frame's (x, uR or NaN, y) triples and has_depth
//                                      flags out - what StereoFrontEnd::process hands on, without the right image's extraction and the match.
// Images are (const uint8_t*, row stride) where the reference has a cv::Mat.  A failed call returns false, never throws, and reports the
// library's message through `error`.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../sship.h"

namespace superslam_hip {

struct StereoSearchParams {
  int half_window = 5;       // the patch is (2 * half_window + 1)^2 pixels; 1 .. 7
  int min_disparity = 0;     // disparities min_disparity .. max_disparity are searched: 3 .. 512 of them
  int max_disparity = 128;
  int uniqueness = 10;       // percent the best cost must stay below the best one further than 1 px away; 0 is off; 0 .. 99
  float min_texture = 0.f;   // texture gate on the left patch's standard deviation in grey levels; <= 0 is off
  float max_rms = 0.f;       // cost gate on the zero-mean RMS difference in grey levels; <= 0 is off
  int lr_check = 1;          // largest accepted |e* - d*| of the left-right check; -1 is off; -1 .. 16
  sship_stereo_search_params c() const {
    return sship_stereo_search_params{half_window, min_disparity, max_disparity, uniqueness, min_texture, max_rms, lr_check};
  }
};

// left / right [h, *_stride bytes] u8, keypoints [n] x kp_stride floats with (x, y) first (kp_stride >= 2).  stereo_out / has_depth_out
// receive n entries each; status (SSHIP_SEARCH_STATUS_*) and cost (C_d*, -1 where no search ran) are optional.
inline bool search_stereo(const uint8_t* left, int left_stride, const uint8_t* right, int right_stride, int h, int w,
                          const std::vector<float>& keypoints, int kp_stride, const StereoSearchParams& params, std::vector<float>& stereo_out,
                          std::vector<uint8_t>& has_depth_out, std::vector<uint8_t>* status = nullptr, std::vector<int64_t>* cost = nullptr,
                          std::string* error = nullptr) {
  if (kp_stride < 2 || keypoints.size() % static_cast<size_t>(kp_stride) != 0 || keypoints.size() / static_cast<size_t>(kp_stride) > 4096) {
    if (error) *error = "search_stereo: keypoints must hold kp_stride >= 2 floats per keypoint, at most 4096 of them";
    return false;
  }
  const size_t n = keypoints.size() / static_cast<size_t>(kp_stride);
  std::vector<float> so(n * 3);
  std::vector<uint8_t> ho(n), st(n);
  std::vector<int64_t> co(n);
  const sship_stereo_search_params p = params.c();
  if (sship_stereo_search_host(left, left_stride, right, right_stride, h, w, keypoints.data(), kp_stride, static_cast<int>(n), &p, so.data(),
                               ho.data(), st.data(), co.data()) != SSHIP_OK) {
    if (error) *error = sship_last_error();
    return false;
  }
  stereo_out.swap(so);
  has_depth_out.swap(ho);
  if (status) status->swap(st);
  if (cost) cost->swap(co);
  return true;
}

}  // namespace superslam_hip
