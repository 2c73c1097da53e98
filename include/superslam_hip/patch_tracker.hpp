// superslam_hip/patch_tracker.hpp - the keypoints of one image carried into another by a bounded 2-D patch search
// (include/sship.h "Patch tracking"):
//   superslam_hip::PatchTrackParams  the library's sship_patch_track_params with its defaults
//   superslam_hip::track_patches     one pair from host arrays: the keyframe's (or the previous frame's) keypoints in, the new frame's
//                                    (x', y', score) rows and matches0 out - an extractor's and a matcher's output for a frame on which
//                                    neither ran.
// Images are (const uint8_t*, row stride) where the reference has a cv::Mat.  A failed call returns false, never throws, and reports the
// library's message through `error`.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../sship.h"

namespace superslam_hip {

struct PatchTrackParams {
  int half_window = 5;       // the patch is (2 * half_window + 1)^2 pixels; 1 .. 7
  int search_radius = 8;     // displacements of up to search_radius pixels per axis around the prediction; 1 .. 16
  int uniqueness = 10;       // percent the best cost must stay below the best one further than 1 px away; 0 is off; 0 .. 99
  float min_texture = 0.f;   // texture gate on the template's standard deviation in grey levels; <= 0 is off
  float max_rms = 0.f;       // cost gate on the zero-mean RMS difference in grey levels; <= 0 is off
  int fb_check = 1;          // largest accepted distance of the forward-backward check; -1 is off; -1 .. 16
  sship_patch_track_params c() const { return sship_patch_track_params{half_window, search_radius, uniqueness, min_texture, max_rms, fb_check}; }
};

// img0 / img1 [h, stride* bytes] u8, keypoints [n] x kp_stride floats with (x, y) first and the score third where kp_stride >= 3
// (kp_stride >= 2); pred: where to centre each search, [n] x pred_stride floats with (px, py) first, or empty for the keypoints themselves.
// kp_out receives n x 3 floats and matches0 n entries; status (SSHIP_TRACK_STATUS_*) and cost (C*, -1 where no search ran) are optional.
inline bool track_patches(const uint8_t* img0, int stride0, const uint8_t* img1, int stride1, int h, int w, const std::vector<float>& keypoints,
                          int kp_stride, const std::vector<float>& pred, int pred_stride, const PatchTrackParams& params,
                          std::vector<float>& kp_out, std::vector<int32_t>& matches0, std::vector<uint8_t>* status = nullptr,
                          std::vector<int64_t>* cost = nullptr, std::string* error = nullptr) {
  if (kp_stride < 2 || keypoints.size() % static_cast<size_t>(kp_stride) != 0 || keypoints.size() / static_cast<size_t>(kp_stride) > 4096) {
    if (error) *error = "track_patches: keypoints must hold kp_stride >= 2 floats per keypoint, at most 4096 of them";
    return false;
  }
  const size_t n = keypoints.size() / static_cast<size_t>(kp_stride);
  if (!pred.empty() && (pred_stride < 2 || pred.size() != n * static_cast<size_t>(pred_stride))) {
    if (error) *error = "track_patches: pred must be empty or hold pred_stride >= 2 floats per keypoint";
    return false;
  }
  std::vector<float> ko(n * 3);
  std::vector<int32_t> mo(n);
  std::vector<uint8_t> st(n);
  std::vector<int64_t> co(n);
  const sship_patch_track_params p = params.c();
  if (sship_patch_track_host(img0, stride0, img1, stride1, h, w, keypoints.data(), kp_stride, pred.empty() ? nullptr : pred.data(), pred_stride,
                             static_cast<int>(n), &p, ko.data(), mo.data(), st.data(), co.data()) != SSHIP_OK) {
    if (error) *error = sship_last_error();
    return false;
  }
  kp_out.swap(ko);
  matches0.swap(mo);
  if (status) status->swap(st);
  if (cost) cost->swap(co);
  return true;
}

}  // namespace superslam_hip
