// Keypoint stereo depth by epipolar search (include/sship.h "Stereo search").
//   k_stereo_search  one wave per keypoint, 4 keypoints per 256-thread workgroup, one launch for the whole batch.
//
// A wave stages the left patch and the right strip pw x (dmax - dlo + pw) of its keypoint in LDS with plain byte loads (nothing is known
// about the alignment of the pointer, the stride or the column), the 64 lanes side by side along the bytes of a row.  Then the lanes share
// the candidates: lane t owns d = dlo + t, dlo + t + 64, ...  The costs are integers, so they are computed in the expanded form, which
// gives the rule's bits:  S1 = sum A - sum R_d,  S2 = sum A^2 + sum R_d^2 - 2 sum A R_d.  sum A and sum A^2 are one wave reduction; sum R_d
// and sum R_d^2 are pw additions of the strip's per-column sums, which the lanes leave in LDS once; the cross term runs on packed bytes:
// the patch rows lie in LDS zero-padded to whole dwords (one broadcast read per dword for the wave), a lane reads the aligned dwords that
// cover its window's row, v_alignbyte_b32 shifts them to the window's first byte and v_dot4_u32_u8 multiplies four pixels at a time (the
// bytes past the window meet the patch's zero padding).  sum A R_d <= 225 x 255^2 < 2^24; N S2 and S1^2 need 64 bits.  The
// smallest minimiser comes from a per-lane scan and a 64-lane butterfly over (C, d); a second butterfly over the candidates further than
// one pixel from d* gives C2; the two neighbours of d* come from the costs the lanes left in LDS.  Every gate is wave-uniform (all lanes
// hold the same sums after a butterfly), so a rejected keypoint's wave simply ends: the waves of a workgroup never wait for each other.
// The left-right check runs the same scan with the roles exchanged and reuses the staging buffers: the right patch at xl - d* is copied
// out of the strip into the patch buffer, the left strip is staged over the right one.  Lane 0 finishes the rule in fp64.
// Dynamic LDS per keypoint, sized on the host from (half_window, candidates): 8 B per candidate, the padded patch, the strip, 6 B per
// strip column for its sums - 3.5 KiB at the defaults, 15.0 KiB at the largest parameters.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "kernels.h"
#include "patch_search.h"

namespace sship {

using namespace patch_search;   // the family's helpers; the 1-D slot, scan and sums below are this kernel's own

namespace {
constexpr int kLanes = kWave;                          // lanes per keypoint: one wave
constexpr int kSlots = 4;                              // keypoints per workgroup
enum { kNone = 0, kFound = 1, kBorder = 2, kRange = 3, kTexture = 4, kEdge = 5, kCost = 6, kAmbiguous = 7, kLrCheck = 8 };

// one keypoint's slot, at the widest strip (every candidate inside the image): byte offsets of the costs (i64 per candidate), the patch
// (rows padded with zeros to nd dwords), the strip (8 bytes of slack: the last window's aligned dwords end past it), the strip's column
// sums of squares (u32) and column sums (u16)
struct SlotLayout { int patch, strip, colq, cols, bytes; };
__host__ __device__ inline SlotLayout slot_layout(int hw, int cand) {
  const int pw = 2 * hw + 1, nd = (pw + 3) / 4, sw = cand + pw - 1;
  SlotLayout l;
  l.patch = round16(8 * cand);
  l.strip = l.patch + round16(pw * 4 * nd);
  l.colq = l.strip + round16(pw * sw + 8);
  l.cols = l.colq + round16(4 * sw);
  l.bytes = l.cols + round16(2 * sw);
  return l;
}

// what a scan reads: the patch (rows of nd dwords), its sums, the strip (row pitch sw bytes) and its column sums
struct ScanIn { const uint8_t* patch; const uint8_t* strip; const uint32_t* colq; const uint16_t* cols; int pw, sw, a1, a2; };

// lane t scans candidates k = t, t + 64, ... < nc: the patch against the window of the strip that starts at column base + step * k.
// The cost of every candidate goes to cost[k] (if not null); (best, bk) is this lane's smallest (C, k), ties to the smaller k.
template <int ND>
__device__ __forceinline__ void scan_candidates(const ScanIn& in, int nc, int base, int step, int t, long long* cost, long long& best, int& bk) {
  const int pw = in.pw, sw = in.sw;
  const long long N = pw * pw;
  best = LLONG_MAX; bk = INT_MAX;
  for (int k = t; k < nc; k += kLanes) {
    const int start = base + step * k;
    int r1 = 0, r2 = 0;
    for (int cc = 0; cc < pw; ++cc) { r1 += in.cols[start + cc]; r2 += (int)in.colq[start + cc]; }
    uint32_t cross = 0;
    for (int r = 0; r < pw; ++r) {
      const int o = r * sw + start;
      const uint32_t* p = reinterpret_cast<const uint32_t*>(in.strip + (o & ~3));
      const uint32_t* a = reinterpret_cast<const uint32_t*>(in.patch + r * 4 * ND);
      const uint32_t sh = (uint32_t)o & 3u;
      uint32_t w0 = p[0];
#pragma unroll
      for (int q = 0; q < ND; ++q) {
        const uint32_t w1 = p[q + 1];
        cross = __builtin_amdgcn_udot4(a[q], __builtin_amdgcn_alignbyte(w1, w0, sh), cross, false);   // bytes sh .. sh + 3 of {w1, w0}
        w0 = w1;
      }
    }
    const int s1 = in.a1 - r1, s2 = in.a2 + r2 - 2 * (int)cross;
    const long long c = N * s2 - (long long)s1 * s1;   // N S2 and S1^2 reach 3.3e9 at w = 7: 64 bits
    if (cost) cost[k] = c;
    if (c < best) { best = c; bk = k; }
  }
}
__device__ __forceinline__ void scan_candidates(const ScanIn& in, int nc, int base, int step, int t, long long* cost, long long& best, int& bk) {
  switch ((in.pw + 3) / 4) {
    case 1: scan_candidates<1>(in, nc, base, step, t, cost, best, bk); break;
    case 2: scan_candidates<2>(in, nc, base, step, t, cost, best, bk); break;
    case 3: scan_candidates<3>(in, nc, base, step, t, cost, best, bk); break;
    default: scan_candidates<4>(in, nc, base, step, t, cost, best, bk); break;
  }
}

// per-column sums of the strip, a lane per column
__device__ __forceinline__ void column_sums(const uint8_t* strip, int pw, int sw, int t, uint32_t* colq, uint16_t* cols) {
  for (int j = t; j < sw; j += kLanes) {
    int s1 = 0, s2 = 0;
    for (int r = 0; r < pw; ++r) { const int v = strip[r * sw + j]; s1 += v; s2 += v * v; }
    cols[j] = (uint16_t)s1; colq[j] = (uint32_t)s2;   // <= 15 x 255 and 15 x 255^2
  }
}

// pw rows of `width` bytes from src (row pitch `stride`) to dst (row pitch `width`), the lanes side by side along a row
__device__ __forceinline__ void stage_rows(const uint8_t* __restrict__ src, long long stride, uint8_t* dst, int pw, int width, int t) {
  for (int r = 0; r < pw; ++r, src += stride, dst += width)
    for (int cc = t; cc < width; cc += kLanes) dst[cc] = src[cc];
}
}  // namespace

__global__ __launch_bounds__(kLanes * kSlots) void k_stereo_search(const uint8_t* __restrict__ imgs, int h, int w, long long stride,
                                                                  const uint32_t* __restrict__ kp, const int* __restrict__ lens,
                                                                  int unit_stride, int K, StereoSearchK c, uint32_t* stereo_out,
                                                                  uint8_t* has_depth_out, uint8_t* status_out, long long* cost_out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int pair = blockIdx.x, g = threadIdx.x / kLanes, t = threadIdx.x % kLanes;
  const int i = blockIdx.y * kSlots + g;
  if (i >= K) return;                                   // wave-uniform, and no workgroup barrier follows
  const int hw = c.half_window, pw = 2 * hw + 1, cand = c.dhi - c.dlo + 1;
  const SlotLayout lay = slot_layout(hw, cand);
  uint8_t* slot = smem + (size_t)g * lay.bytes;
  long long* costs = reinterpret_cast<long long*>(slot);
  uint8_t* patch = slot + lay.patch;
  uint8_t* strip = slot + lay.strip;
  uint32_t* colq = reinterpret_cast<uint32_t*>(slot + lay.colq);
  uint16_t* cols = reinterpret_cast<uint16_t*>(slot + lay.cols);
  const int pitch = 4 * ((pw + 3) / 4);                  // bytes of a patch row in LDS
  ScanIn in{patch, strip, colq, cols, pw, 0, 0, 0};
  const size_t row = (size_t)pair * K + i, unit = (size_t)pair * unit_stride;

  uint32_t bx = 0, by = 0, out_r = kQuietNan;
  int status = kNone, hd = 0;
  long long cost = -1;
  const int n0 = min(max(lens[unit], 0), K);
  if (i < n0) {
    // steps 2-3
    bx = kp[(unit * K + i) * 3]; by = kp[(unit * K + i) * 3 + 1];
    const float x = __uint_as_float(bx), y = __uint_as_float(by);
    status = kBorder;
    int xl = 0, yl = 0, nc = 0;
    if (coord_ok(x) && coord_ok(y)) {
      xl = (int)floor((double)x + 0.5); yl = (int)floor((double)y + 0.5);
      if (xl - hw >= 0 && xl + hw < w && yl - hw >= 0 && yl + hw < h) {
        nc = min(c.dhi, xl - hw) - c.dlo + 1;
        status = nc < 3 ? kRange : kFound;
      }
    }
    if (status == kFound) {
      // stage the left patch and the right strip: column j of the strip is image column xl - dmax - hw + j, so candidate k = d - dlo
      // starts at column nc - 1 - k
      const int sw = nc + pw - 1, dmax = c.dlo + nc - 1;
      const uint8_t* il = imgs + ((size_t)(2 * pair) * h + (yl - hw)) * stride;
      const uint8_t* ir = il + (size_t)h * stride;
      stage_patch(il + (xl - hw), stride, patch, pw, pitch, t);
      stage_rows(ir + (xl - dmax - hw), stride, strip, pw, sw, t);
      wave_sync();
      patch_sums(patch, pw * pitch, t, in.a1, in.a2);
      // step 4
      if (c.tex) {
        const long long T = (long long)(pw * pw) * in.a2 - (long long)in.a1 * in.a1;
        if ((double)T < c.tex2) status = kTexture;
      }
    }
    if (status == kFound) {
      // steps 5-8
      const int sw = nc + pw - 1;
      long long best; int ks;
      column_sums(strip, pw, sw, t, colq, cols);
      wave_sync();
      in.sw = sw;
      scan_candidates(in, nc, nc - 1, -1, t, costs, best, ks);
      wave_argmin(best, ks);
      cost = best;
      wave_sync();                                      // the costs of the other lanes are read below
      if (ks == 0 || ks == nc - 1) status = kEdge;
      else if (c.gate && (double)cost > c.gate2) status = kCost;
      else if (c.uniqueness > 0) {
        long long c2 = LLONG_MAX;
        for (int k = t; k < nc; k += kLanes)
          if (k < ks - 1 || k > ks + 1) c2 = min(c2, costs[k]);
#pragma unroll
        for (int m = kLanes / 2; m >= 1; m >>= 1) c2 = min(c2, (long long)__shfl_xor(c2, m, kLanes));
        if (c2 != LLONG_MAX && !(100 * cost < (long long)(100 - c.uniqueness) * c2)) status = kAmbiguous;
      }
      if (status == kFound && c.lr >= 0) {
        // step 9: the right patch at xr leaves the strip, the left strip [xr + dlo - hw, xr + emax + hw] takes its place
        const int xr = xl - (c.dlo + ks), ne = min(c.dhi, w - 1 - hw - xr) - c.dlo + 1, sw2 = ne + pw - 1;
        uint8_t keep[4];                                // pw^2 <= 225 < 4 * 64
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = t + q * kLanes;
          keep[q] = k < pw * pw ? strip[(k / pw) * sw + (nc - 1 - ks) + k % pw] : 0;
        }
        wave_sync();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = t + q * kLanes;
          if (k < pw * pw) patch[(k / pw) * pitch + k % pw] = keep[q];   // the padding stays zero
        }
        const uint8_t* il = imgs + ((size_t)(2 * pair) * h + (yl - hw)) * stride;
        stage_rows(il + (xr + c.dlo - hw), stride, strip, pw, sw2, t);
        wave_sync();
        patch_sums(patch, pw * pitch, t, in.a1, in.a2);
        column_sums(strip, pw, sw2, t, colq, cols);
        wave_sync();
        in.sw = sw2;
        long long b; int es;
        scan_candidates(in, ne, 0, 1, t, nullptr, b, es);
        wave_argmin(b, es);
        if (abs(es - ks) > c.lr) status = kLrCheck;
      }
      if (status == kFound) {
        // step 10: den >= 1 (the left neighbour of the smallest minimiser is strictly larger)
        const long long cm = costs[ks - 1], cp = costs[ks + 1];
        const long long den = cm + cp - 2 * cost;
        const double delta = (double)(cm - cp) / (double)(2 * den);
        out_r = __float_as_uint((float)(((double)x - (double)(c.dlo + ks)) - delta));
        hd = 1;
      }
    }
  }
  if (t != 0) return;
  stereo_out[row * 3] = bx; stereo_out[row * 3 + 1] = out_r; stereo_out[row * 3 + 2] = by;
  has_depth_out[row] = (uint8_t)hd;
  if (status_out) status_out[row] = (uint8_t)status;
  if (cost_out) cost_out[row] = cost;
}

void launch_stereo_search(const uint8_t* imgs, int pairs, int h, int w, long long stride, const float* kp, const int* lens, int unit_stride,
                          int max_kp, const StereoSearchK& c, float* stereo_out, uint8_t* has_depth_out, uint8_t* status, long long* cost,
                          hipStream_t s) {
  const size_t smem = (size_t)kSlots * slot_layout(c.half_window, c.dhi - c.dlo + 1).bytes;   // 61 632 B at the largest parameters
  hipLaunchKernelGGL(k_stereo_search, dim3(pairs, (max_kp + kSlots - 1) / kSlots), dim3(kLanes * kSlots), smem, s, imgs, h, w, stride,
                     reinterpret_cast<const uint32_t*>(kp), lens, unit_stride, max_kp, c, reinterpret_cast<uint32_t*>(stereo_out),
                     has_depth_out, status, cost);
}

}  // namespace sship
