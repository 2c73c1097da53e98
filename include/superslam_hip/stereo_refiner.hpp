// superslam_hip/stereo_refiner.hpp - sub-pixel uR by patch correlation in the rectified pair (include/sship.h "Stereo refinement"):
//   superslam_hip::StereoRefineParams  the library's sship_stereo_refine_params with its defaults
//   superslam_hip::refine_stereo       one pair from host arrays, the step after one StereoFrontEnd::process: the frame's (uL, uR, vL)
//                                      triples and has_depth flags in, the refined ones out.
// Images are (const uint8_t*, row stride) where the reference has a cv::Mat.  A failed call returns false, never throws, and reports the
// library's message through `error`.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../sship.h"

namespace superslam_hip {

struct StereoRefineParams {
  int half_window = 5;         // the patch is (2 * half_window + 1)^2 pixels; 1 .. 7
  int search_radius = 5;       // offsets -search_radius .. +search_radius are searched; 1 .. 15
  float max_rms = 0.f;         // cost gate on the zero-mean RMS difference in grey levels; <= 0 is off
  float min_disparity = 0.f;   // smallest accepted refined disparity
  int on_reject = SSHIP_REFINE_KEEP;   // SSHIP_REFINE_KEEP: a rejected row keeps its input; SSHIP_REFINE_DROP: it loses its depth
  sship_stereo_refine_params c() const { return sship_stereo_refine_params{half_window, search_radius, max_rms, min_disparity, on_reject}; }
};

// left / right [h, *_stride bytes] u8, stereo [n] x (uL, uR or NaN, vL), has_depth [n].  stereo_out / has_depth_out receive n entries each
// (they may be the input vectors); status (SSHIP_REFINE_STATUS_*) and cost (C_k*, -1 where no search ran) are optional.
inline bool refine_stereo(const uint8_t* left, int left_stride, const uint8_t* right, int right_stride, int h, int w,
                          const std::vector<float>& stereo, const std::vector<uint8_t>& has_depth, const StereoRefineParams& params,
                          std::vector<float>& stereo_out, std::vector<uint8_t>& has_depth_out, std::vector<uint8_t>* status = nullptr,
                          std::vector<int64_t>* cost = nullptr, std::string* error = nullptr) {
  const size_t n = has_depth.size();
  if (stereo.size() != n * 3 || n > 4096) {
    if (error) *error = "refine_stereo: stereo must hold 3 floats per has_depth entry, at most 4096 of them";
    return false;
  }
  std::vector<float> so(n * 3);
  std::vector<uint8_t> ho(n), st(n);
  std::vector<int64_t> co(n);
  const sship_stereo_refine_params p = params.c();
  if (sship_stereo_refine_host(left, left_stride, right, right_stride, h, w, stereo.data(), has_depth.data(), static_cast<int>(n), &p, so.data(),
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
