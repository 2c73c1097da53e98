// Sub-pixel disparity refinement by patch correlation (include/sship.h "Stereo refinement").
//   k_stereo_refine  one 16-lane group per keypoint slot, 16 slots per 256-thread workgroup, one launch for the whole batch.
//
// The keypoints are scattered over the image, so what a keypoint costs is the cache lines its 2w+1 rows touch, not its arithmetic.  A group
// stages the left patch and the right strip of its keypoint in LDS with plain byte loads (nothing is known about the alignment of the
// pointer, the stride or the column): one pass over the rows, the 16 lanes side by side along the (2w+1) + (2w+1+2L) bytes of a row - two
// full passes of 16 at the defaults.  Then the lanes share the offsets: lane t owns offsets t - L and t + 16 - L (2L+1 <= 31 <= 32) and
// walks the whole window for both, so a left byte is one LDS broadcast for the group and the right bytes of the 16 lanes are neighbours.
// S1, S2 and C_k are integers - any order gives the rule's bits.  The smallest minimiser is found with a 16-lane butterfly over (C, k);
// the two neighbours of k* come from the costs the lanes left in LDS.  Lane 0 of the group finishes the rule in fp64 and writes the row.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "kernels.h"
#include "patch_search.h"

namespace sship {

namespace {
constexpr int kLanes = 16;                             // lanes per keypoint
constexpr int kSlots = 16;                             // keypoints per workgroup
constexpr int kMaxPatch = 2 * 7 + 1;                   // half_window <= 7
constexpr int kMaxStrip = kMaxPatch + 2 * 15;          // search_radius <= 15
struct RefineSlot {
  long long cost[2 * kLanes];
  uint8_t left[(kMaxPatch * kMaxPatch + 3) / 4 * 4];
  uint8_t right[(kMaxPatch * kMaxStrip + 3) / 4 * 4];
};
enum { kNone = 0, kRefined = 1, kBorder = 2, kEdge = 3, kCost = 4, kDisparity = 5 };
using patch_search::coord_ok;
using patch_search::kQuietNan;
}  // namespace

__global__ __launch_bounds__(kLanes * kSlots) void k_stereo_refine(const uint8_t* __restrict__ imgs, int h, int w, long long stride,
                                                                   const uint32_t* stereo_in, const uint8_t* has_depth_in,
                                                                   const int* __restrict__ lens, int n_stride, int R, StereoRefineK c,
                                                                   uint32_t* stereo_out, uint8_t* has_depth_out, uint8_t* status_out,
                                                                   long long* cost_out) {
  __shared__ RefineSlot slots[kSlots];
  const int pair = blockIdx.x, g = threadIdx.x / kLanes, t = threadIdx.x % kLanes;
  const int i = blockIdx.y * kSlots + g;
  RefineSlot& s = slots[g];
  const int hw = c.half_window, L = c.search_radius, pw = 2 * hw + 1, rw = pw + 2 * L, nk = 2 * L + 1;
  const size_t row = (size_t)pair * R + (i < R ? i : R - 1);

  // steps 1-3: every lane of the group reads the row (before any lane writes it: the call may be in place)
  uint32_t bu = 0, br = kQuietNan, bv = 0;
  int status = kNone, hd = 0, xl = 0, xr = 0, y = 0;
  bool search = false;
  if (i < R && i < min(max(lens[(size_t)pair * n_stride], 0), R)) {
    bu = stereo_in[row * 3]; bv = stereo_in[row * 3 + 2];
    if (has_depth_in[row]) {
      br = stereo_in[row * 3 + 1];
      hd = 1;
      status = kBorder;
      const float uL = __uint_as_float(bu), uR = __uint_as_float(br), vL = __uint_as_float(bv);
      if (coord_ok(uL) && coord_ok(uR) && coord_ok(vL)) {
        xl = (int)floor((double)uL + 0.5); xr = (int)floor((double)uR + 0.5); y = (int)floor((double)vL + 0.5);
        search = xl - hw >= 0 && xl + hw < w && y - hw >= 0 && y + hw < h && xr - L - hw >= 0 && xr + L + hw < w;
      }
    }
  }

  // stage (2w+1) rows: the left patch and the right strip of a row side by side along the lanes
  if (search) {
    const uint8_t* rl = imgs + ((size_t)(2 * pair) * h + (y - hw)) * stride + (xl - hw);
    const uint8_t* rr = imgs + ((size_t)(2 * pair + 1) * h + (y - hw)) * stride + (xr - L - hw);
    for (int r = 0; r < pw; ++r, rl += stride, rr += stride)
      for (int cc = t; cc < pw + rw; cc += kLanes) {
        if (cc < pw) s.left[r * pw + cc] = rl[cc];
        else s.right[r * rw + (cc - pw)] = rr[cc - pw];
      }
  }
  __syncthreads();

  // step 4: lane t owns offsets j0 = t and j1 = t + 16 (as indices k + L); an index past 2L repeats the last one and is thrown away
  long long c0 = LLONG_MAX, c1 = LLONG_MAX;
  const int j0 = t, j1 = t + kLanes;
  if (search) {
    const int o0 = min(j0, nk - 1), o1 = min(j1, nk - 1);
    int a1 = 0, a2 = 0, b1 = 0, b2 = 0;
    for (int r = 0; r < pw; ++r) {
      const uint8_t* lp = s.left + r * pw;
      const uint8_t* rp = s.right + r * rw;
      for (int cc = 0; cc < pw; ++cc) {
        const int l = lp[cc], d0 = l - rp[cc + o0], d1 = l - rp[cc + o1];
        a1 += d0; a2 += d0 * d0;
        b1 += d1; b2 += d1 * d1;
      }
    }
    const long long N = pw * pw;
    if (j0 < nk) c0 = N * a2 - (long long)a1 * a1;      // S1^2 reaches 3.3e9 at w = 7: 64 bits
    if (j1 < nk) c1 = N * b2 - (long long)b1 * b1;
    s.cost[j0] = c0; s.cost[j1] = c1;
  }
  // step 5: the smallest index attaining the minimum, over the 16 lanes of the group (every lane of the wave takes part in the shuffles)
  long long best = c0;
  int bj = j0;
  if (c1 < best) { best = c1; bj = j1; }
#pragma unroll
  for (int m = kLanes / 2; m >= 1; m >>= 1) {
    const long long oc = __shfl_xor(best, m, kLanes);
    const int oj = __shfl_xor(bj, m, kLanes);
    if (oc < best || (oc == best && oj < bj)) { best = oc; bj = oj; }
  }
  __syncthreads();
  if (t != 0 || i >= R) return;

  long long cost = -1;
  uint32_t out_r = br;
  if (search) {
    cost = best;
    if (bj == 0 || bj == nk - 1) status = kEdge;
    else if (c.gate && (double)cost > c.gate2) status = kCost;
    else {
      // steps 6-8: den >= 1 (the left neighbour of the smallest minimiser is strictly larger)
      const long long cm = s.cost[bj - 1], cp = s.cost[bj + 1];
      const long long den = cm + cp - 2 * cost;
      const double delta = (double)(cm - cp) / (double)(2 * den);
      const float uL = __uint_as_float(bu);
      const float un = (float)(((double)uL - (double)(xl - xr - (bj - L))) + delta);
      if (uL - un >= c.min_disparity) { status = kRefined; out_r = __float_as_uint(un); }
      else status = kDisparity;
    }
    if (status >= kEdge && c.drop) { out_r = kQuietNan; hd = 0; }
  }
  stereo_out[row * 3] = bu; stereo_out[row * 3 + 1] = out_r; stereo_out[row * 3 + 2] = bv;
  has_depth_out[row] = (uint8_t)hd;
  if (status_out) status_out[row] = (uint8_t)status;
  if (cost_out) cost_out[row] = cost;
}

void launch_stereo_refine(const uint8_t* imgs, int pairs, int h, int w, long long stride, const float* stereo_in, const uint8_t* has_depth_in,
                          const int* lens, int n_stride, int max_kp, const StereoRefineK& c, float* stereo_out, uint8_t* has_depth_out,
                          uint8_t* status, long long* cost, hipStream_t s) {
  hipLaunchKernelGGL(k_stereo_refine, dim3(pairs, (max_kp + kSlots - 1) / kSlots), dim3(kLanes * kSlots), 0, s, imgs, h, w, stride,
                     reinterpret_cast<const uint32_t*>(stereo_in), has_depth_in, lens, n_stride, max_kp, c,
                     reinterpret_cast<uint32_t*>(stereo_out), has_depth_out, status, cost);
}

}  // namespace sship
