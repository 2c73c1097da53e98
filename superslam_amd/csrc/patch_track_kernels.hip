// Keypoint tracking by 2-D patch search (include/sship.h "Patch tracking"): the temporal twin of the stereo search.
//   k_patch_track  one wave per keypoint, 3 keypoints per 192-thread workgroup, one launch for the whole batch.
//
// A wave stages the template of its keypoint (a pw x pw patch of I0) and the (ncx + pw - 1) x (ncy + pw - 1) region of I1 that holds every
// candidate patch of the clipped search box in LDS with plain byte loads (nothing is known about the alignment of the pointers, the strides
// or the columns).  Then the lanes share the candidates: lane t owns k = t, t + 64, ... in the rule's order k = (dy - loy) ncx + (dx - lox).
// The costs are integers, so they are computed in the expanded form, which gives the rule's bits:  S1 = sum A - sum B,  S2 = sum A^2 +
// sum B^2 - 2 sum A B.  sum A and sum A^2 are one wave reduction; sum B and sum B^2 of a window are separable: the lanes leave the sums of
// the pw bytes right of every region byte in LDS once (a row of ncx sums per region row), a candidate adds pw of them down its column.
// The cross term runs on packed bytes as in the stereo search: the template rows lie in LDS zero-padded to whole dwords, a lane reads the
// aligned dwords that cover its window's row, v_alignbyte_b32 shifts them to the window's first byte and v_dot4_u32_u8 multiplies four
// pixels at a time (the bytes past the window meet the template's zero padding).  sum A B <= 225 x 255^2 < 2^24; N S2 and S1^2 need 64
// bits.  The smallest minimiser comes from a per-lane scan and a 64-lane butterfly over (C, k); a second butterfly over the candidates
// further than one pixel from (dx*, dy*) gives C2; the four neighbours of the minimiser come from the costs the lanes left in LDS.  Every
// gate is wave-uniform (all lanes hold the same sums after a butterfly), so a rejected keypoint's wave simply ends: the waves of a
// workgroup never wait for each other.  The forward-backward check runs the same scan with the roles exchanged and reuses the staging
// buffers: the I1 patch at the minimiser is copied out of the region into the template buffer, the I0 region is staged over the I1 one
// (its candidates run against the pixels: e = ex_hi first column, so the scan walks the region backwards).  The fit is fp64.
// Dynamic LDS per keypoint, sized on the host from (half_window, search_radius) at the unclipped box: 8 B per candidate, the padded template,
// the region + 8 B, 6 B per (region row, box column) - 5 984 B at the defaults, 20 496 B at the largest parameters.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "patch_search.h"

namespace sship {

using namespace patch_search;
using namespace patch_search::search2d;

namespace {
constexpr int kLanes = kWave;                          // lanes per keypoint: one wave
constexpr int kSlots = 3;                              // keypoints per workgroup: 3 x 20 496 B = 61 488 B at half_window 7, search_radius 16
}  // namespace

// The per-keypoint body is patch_search.h's track_level, on the pair's two images.  pred and kp_out may be the same array (no __restrict__
// on either): a wave reads its row of pred before lane 0 writes that row of kp_out, and no other wave touches the row
__global__ __launch_bounds__(kLanes * kSlots) void k_patch_track(const uint8_t* __restrict__ imgs0, long long image_stride0, long long stride0,
                                                                const uint8_t* __restrict__ imgs1, long long image_stride1, long long stride1,
                                                                int h, int w, const uint32_t* kp, const int* __restrict__ lens, int unit_stride,
                                                                const uint32_t* pred, int K, PatchTrackK c, uint32_t* kp_out, int* n_out,
                                                                int* matches_out, uint8_t* status_out, long long* cost_out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int pair = blockIdx.x, g = threadIdx.x / kLanes, t = threadIdx.x % kLanes;
  const int i = blockIdx.y * kSlots + g;
  if (i >= K) return;                                   // wave-uniform, and no workgroup barrier follows
  uint8_t* slot = smem + (size_t)g * slot_layout(c.half_window, c.radius).bytes;
  const size_t row = (size_t)pair * K + i, unit = (size_t)pair * unit_stride;

  uint32_t out_x = 0, out_y = 0, score = 0;
  int status = kNone, match = -1;
  long long cost = -1;
  const int n0 = min(max(lens[unit], 0), K);
  if (n_out && i == 0 && t == 0) n_out[pair] = n0;
  if (i < n0) {
    const float x = __uint_as_float(kp[(unit * K + i) * 3]), y = __uint_as_float(kp[(unit * K + i) * 3 + 1]);
    score = kp[(unit * K + i) * 3 + 2];
    const float px = pred ? __uint_as_float(pred[row * 3]) : x, py = pred ? __uint_as_float(pred[row * 3 + 1]) : y;
    const LevelOut o = track_level(imgs0 + (size_t)pair * image_stride0, stride0, imgs1 + (size_t)pair * image_stride1, stride1, h, w, x, y, px, py,
                                   c, slot, t);
    status = o.status; cost = o.cost; out_x = o.x; out_y = o.y;
    if (status == kTracked) match = i;
  }
  if (t != 0) return;
  kp_out[row * 3] = out_x; kp_out[row * 3 + 1] = out_y; kp_out[row * 3 + 2] = score;
  matches_out[row] = match;
  if (status_out) status_out[row] = (uint8_t)status;
  if (cost_out) cost_out[row] = cost;
}

void launch_patch_track(const uint8_t* imgs0, long long image_stride0, int stride0, const uint8_t* imgs1, long long image_stride1, int stride1,
                        int pairs, int h, int w, const float* kp, const int* lens, int unit_stride, const float* pred, int max_kp,
                        const PatchTrackK& c, float* kp_out, int* n_out, int* matches0, uint8_t* status, long long* cost, hipStream_t s) {
  const size_t smem = (size_t)kSlots * slot_layout(c.half_window, c.radius).bytes;   // 61 488 B at the largest parameters
  hipLaunchKernelGGL(k_patch_track, dim3(pairs, (max_kp + kSlots - 1) / kSlots), dim3(kLanes * kSlots), smem, s, imgs0, image_stride0,
                     (long long)stride0, imgs1, image_stride1, (long long)stride1, h, w, reinterpret_cast<const uint32_t*>(kp), lens, unit_stride,
                     reinterpret_cast<const uint32_t*>(pred), max_kp, c, reinterpret_cast<uint32_t*>(kp_out), n_out, matches0, status, cost);
}

}  // namespace sship
