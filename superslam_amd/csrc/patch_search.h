// The wave-per-keypoint patch search, shared by the kernels that run one: the stereo search (stereo_search_kernels.hip), the patch tracker
// (patch_track_kernels.hip, whose header comment explains the method) and the pyramid tracker (pyr_kernels.hip).  Device code: only .hip
// files include it.  namespace patch_search holds what the whole family uses - the stereo refinement (16 lanes per keypoint) takes
// coord_ok and kQuietNan from it and nothing else; namespace patch_search::search2d holds the 2-D search, steps 2 to 10 of the
// patch-tracking rule (include/sship.h "Patch tracking") as one device function of one level.  The 1-D search of the stereo kernels keeps
// its own slot, scan and sums under the same names, which is why the 2-D ones live in a namespace of their own.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "kernels.h"

namespace sship {
namespace patch_search {

constexpr uint32_t kQuietNan = 0x7fc00000u;

__host__ __device__ inline int round16(int v) { return (v + 15) & ~15; }

__device__ inline bool coord_ok(float x) { return x >= 0.f && x < 16384.f; }   // NaN and +-inf: false

// the lanes of one wave exchange data through LDS: order this wave's LDS traffic
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the smallest (C, k) over the wave, ties to the smaller k; every lane ends with the result
__device__ __forceinline__ void wave_argmin(long long& best, int& bk) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    const long long oc = __shfl_xor(best, m, kWave);
    const int ok = __shfl_xor(bk, m, kWave);
    if (oc < best || (oc == best && ok < bk)) { best = oc; bk = ok; }
  }
}

// sum and sum of squares of the template over the wave (the padding is zero); every lane ends with the result
__device__ __forceinline__ void patch_sums(const uint8_t* patch, int bytes, int t, int& a1, int& a2) {
  a1 = 0; a2 = 0;
  for (int k = t; k < bytes; k += kWave) { const int a = patch[k]; a1 += a; a2 += a * a; }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) { a1 += __shfl_xor(a1, m, kWave); a2 += __shfl_xor(a2, m, kWave); }
}

// the template: pw rows of pw bytes from src to rows of `pitch` >= pw bytes, the rest of a row zero
__device__ __forceinline__ void stage_patch(const uint8_t* __restrict__ src, long long stride, uint8_t* dst, int pw, int pitch, int t) {
  for (int k = t; k < pw * pitch; k += kWave) {
    const int r = k / pitch, cc = k % pitch;
    dst[k] = cc < pw ? src[r * stride + cc] : (uint8_t)0;
  }
}

namespace search2d {

enum { kNone = 0, kTracked = 1, kBorder = 2, kRange = 3, kTexture = 4, kEdge = 5, kCost = 6, kAmbiguous = 7, kFbCheck = 8 };

// one keypoint's slot, at the unclipped box of nb = 2 R + 1 candidates a side: byte offsets of the costs (i64 per candidate, at 0), the
// template (rows padded with zeros to nd dwords), the region (8 bytes of slack: the last window's aligned dwords end past it), and the
// row sums of squares (u32) and of pixels (u16) per (region row, box column)
struct SlotLayout { int patch, region, hq, hs, bytes; };
__host__ __device__ inline SlotLayout slot_layout(int hw, int radius) {
  const int pw = 2 * hw + 1, nd = (pw + 3) / 4, nb = 2 * radius + 1, rw = nb + pw - 1;
  SlotLayout l;
  l.patch = round16(8 * nb * nb);
  l.region = l.patch + round16(pw * 4 * nd);
  l.hq = l.region + round16(rw * rw + 8);
  l.hs = l.hq + round16(4 * rw * nb);
  l.bytes = l.hs + round16(2 * rw * nb);
  return l;
}

// what a scan reads: the template (rows of nd dwords) and its sums, the region (row pitch rw bytes) and its row sums (row pitch ncx entries)
struct ScanIn { const uint8_t* patch; const uint8_t* region; const uint32_t* hq; const uint16_t* hs; int pw, rw, ncx, a1, a2; };

// lane t scans candidates k = t, t + 64, ... < nc in the rule's order k = ky ncx + kx: the template against the window of the region whose
// first byte is at row base_y + step ky, column base_x + step kx.  The cost of every candidate goes to cost[k] (if not null); (best, bk) is
// this lane's smallest (C, k), ties to the smaller k.
template <int ND>
__device__ __forceinline__ void scan_candidates(const ScanIn& in, int nc, int base_x, int base_y, int step, int t, long long* cost, long long& best,
                                                int& bk) {
  const int pw = in.pw, rw = in.rw, ncx = in.ncx;
  const long long N = pw * pw;
  best = LLONG_MAX; bk = INT_MAX;
  for (int k = t; k < nc; k += kWave) {
    const int ky = k / ncx, kx = k - ky * ncx;
    const int col = base_x + step * kx, row = base_y + step * ky;
    int r1 = 0, r2 = 0;
    uint32_t cross = 0;
    for (int r = 0; r < pw; ++r) {
      r1 += in.hs[(row + r) * ncx + col]; r2 += (int)in.hq[(row + r) * ncx + col];
      const int o = (row + r) * rw + col;
      const uint32_t* p = reinterpret_cast<const uint32_t*>(in.region + (o & ~3));
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
__device__ __forceinline__ void scan_candidates(const ScanIn& in, int nc, int base_x, int base_y, int step, int t, long long* cost, long long& best,
                                                int& bk) {
  switch ((in.pw + 3) / 4) {
    case 1: scan_candidates<1>(in, nc, base_x, base_y, step, t, cost, best, bk); break;
    case 2: scan_candidates<2>(in, nc, base_x, base_y, step, t, cost, best, bk); break;
    case 3: scan_candidates<3>(in, nc, base_x, base_y, step, t, cost, best, bk); break;
    default: scan_candidates<4>(in, nc, base_x, base_y, step, t, cost, best, bk); break;
  }
}

// hs / hq [r ncx + c] = the sum (of squares) of the pw region bytes of row r from column c on, r < rh, c < ncx: a lane per entry
__device__ __forceinline__ void row_sums(const uint8_t* region, int pw, int rw, int rh, int ncx, int t, uint32_t* hq, uint16_t* hs) {
  for (int k = t; k < rh * ncx; k += kWave) {
    const int r = k / ncx, cc = k - r * ncx;
    const uint8_t* p = region + r * rw + cc;
    int s1 = 0, s2 = 0;
    for (int q = 0; q < pw; ++q) { const int v = p[q]; s1 += v; s2 += v * v; }
    hs[k] = (uint16_t)s1; hq[k] = (uint32_t)s2;          // <= 15 x 255 and 15 x 255^2
  }
}

// rh rows of rw bytes from src (row pitch `stride`) to dst (row pitch rw), the lanes side by side along the bytes of the region
__device__ __forceinline__ void stage_region(const uint8_t* __restrict__ src, long long stride, uint8_t* dst, int rh, int rw, int t) {
  for (int k = t; k < rh * rw; k += kWave) {
    const int r = k / rw, cc = k - r * rw;
    dst[k] = src[r * stride + cc];
  }
}

struct LevelOut { int status; long long cost; uint32_t x, y; };   // x, y: the bits of (x', y'), quiet NaNs unless the status is TRACKED

// steps 2 to 10 of the patch-tracking rule for one keypoint inside the count, on the images (i0p, i1p) of h x w pixels, by one wave whose
// LDS slot (slot_layout(c.half_window, c.radius).bytes) is `slot`.  (x, y) is the keypoint, (px, py) the prediction.  Every lane returns
// the same values.  The template is read only after step 2 found it inside I0, the region only after step 3 found a box of at least 3 x 3
// candidates whose patches lie inside I1: no load leaves an image.
__device__ __forceinline__ LevelOut track_level(const uint8_t* __restrict__ i0p, long long stride0, const uint8_t* __restrict__ i1p, long long stride1,
                                                int h, int w, float x, float y, float px, float py, const PatchTrackK& c, uint8_t* slot, int t) {
  const int hw = c.half_window, R = c.radius, pw = 2 * hw + 1;
  const SlotLayout lay = slot_layout(hw, R);
  long long* costs = reinterpret_cast<long long*>(slot);
  uint8_t* patch = slot + lay.patch;
  uint8_t* region = slot + lay.region;
  uint32_t* hq = reinterpret_cast<uint32_t*>(slot + lay.hq);
  uint16_t* hs = reinterpret_cast<uint16_t*>(slot + lay.hs);
  const int pitch = 4 * ((pw + 3) / 4);                  // bytes of a template row in LDS
  ScanIn in{patch, region, hq, hs, pw, 0, 0, 0, 0};
  LevelOut o{kBorder, -1, kQuietNan, kQuietNan};
  int xa = 0, ya = 0, xp = 0, yp = 0, lox = 0, loy = 0, ncx = 0, ncy = 0;
  // step 2
  if (coord_ok(x) && coord_ok(y) && coord_ok(px) && coord_ok(py)) {
    xa = (int)floor((double)x + 0.5); ya = (int)floor((double)y + 0.5);
    xp = (int)floor((double)px + 0.5); yp = (int)floor((double)py + 0.5);
    if (xa - hw >= 0 && xa + hw < w && ya - hw >= 0 && ya + hw < h) {
      // step 3: every candidate patch inside I1
      lox = max(-R, hw - xp); loy = max(-R, hw - yp);
      ncx = min(R, w - 1 - hw - xp) - lox + 1; ncy = min(R, h - 1 - hw - yp) - loy + 1;
      o.status = (ncx < 3 || ncy < 3) ? kRange : kTracked;
    }
  }
  if (o.status == kTracked) {
    // stage the template and the region of I1: byte (r, j) of the region is pixel (yp + loy - hw + r, xp + lox - hw + j), so candidate
    // (kx, ky) = (dx - lox, dy - loy) starts at row ky, column kx
    const uint8_t* i0 = i0p + (size_t)(ya - hw) * stride0 + (xa - hw);
    const uint8_t* i1 = i1p + (size_t)(yp + loy - hw) * stride1 + (xp + lox - hw);
    stage_patch(i0, stride0, patch, pw, pitch, t);
    stage_region(i1, stride1, region, ncy + pw - 1, ncx + pw - 1, t);
    wave_sync();
    patch_sums(patch, pw * pitch, t, in.a1, in.a2);
    // step 4
    if (c.tex) {
      const long long T = (long long)(pw * pw) * in.a2 - (long long)in.a1 * in.a1;
      if ((double)T < c.tex2) o.status = kTexture;
    }
  }
  if (o.status != kTracked) return o;
  // steps 5-8
  const int rw = ncx + pw - 1, rh = ncy + pw - 1, nc = ncx * ncy;
  long long best; int ks;
  row_sums(region, pw, rw, rh, ncx, t, hq, hs);
  wave_sync();
  in.rw = rw; in.ncx = ncx;
  scan_candidates(in, nc, 0, 0, 1, t, costs, best, ks);
  wave_argmin(best, ks);
  const long long cost = best;
  o.cost = cost;
  wave_sync();                                          // the costs of the other lanes are read below
  const int kys = ks / ncx, kxs = ks - kys * ncx;
  const int dxs = lox + kxs, dys = loy + kys;
  if (kxs == 0 || kxs == ncx - 1 || kys == 0 || kys == ncy - 1) o.status = kEdge;
  else if (c.gate && (double)cost > c.gate2) o.status = kCost;
  else if (c.uniqueness > 0) {
    long long c2 = LLONG_MAX;
    for (int k = t; k < nc; k += kWave) {
      const int ky = k / ncx, kx = k - ky * ncx;
      if (abs(kx - kxs) > 1 || abs(ky - kys) > 1) c2 = min(c2, costs[k]);
    }
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) c2 = min(c2, (long long)__shfl_xor(c2, m, kWave));
    if (c2 != LLONG_MAX && !(100 * cost < (long long)(100 - c.uniqueness) * c2)) o.status = kAmbiguous;
  }
  if (o.status == kTracked && c.fb >= 0) {
    // step 9: the I1 patch at the minimiser leaves the region for the template buffer; the region of I0 that holds the patches at
    // (cx - ex, cy - ey) takes its place, column 0 at cx - ehix - hw: candidate (kx, ky) = (ex - elox, ey - eloy) starts at row
    // nby - 1 - ky, column nbx - 1 - kx
    const int cx = xa + dxs, cy = ya + dys;
    const int elox = max(-R, cx - (w - 1 - hw)), ehix = min(R, cx - hw), eloy = max(-R, cy - (h - 1 - hw)), ehiy = min(R, cy - hw);
    const int nbx = ehix - elox + 1, nby = ehiy - eloy + 1, rw2 = nbx + pw - 1, rh2 = nby + pw - 1;
    uint8_t keep[4];                                    // pw^2 <= 225 < 4 * 64
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = t + q * kWave;
      keep[q] = k < pw * pw ? region[(kys + k / pw) * rw + kxs + k % pw] : 0;
    }
    wave_sync();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = t + q * kWave;
      if (k < pw * pw) patch[(k / pw) * pitch + k % pw] = keep[q];   // the padding stays zero
    }
    const uint8_t* i0 = i0p + (size_t)(cy - ehiy - hw) * stride0 + (cx - ehix - hw);
    stage_region(i0, stride0, region, rh2, rw2, t);
    wave_sync();
    patch_sums(patch, pw * pitch, t, in.a1, in.a2);
    row_sums(region, pw, rw2, rh2, nbx, t, hq, hs);
    wave_sync();
    in.rw = rw2; in.ncx = nbx;
    long long b; int es;
    scan_candidates(in, nbx * nby, nbx - 1, nby - 1, -1, t, nullptr, b, es);
    wave_argmin(b, es);
    const int eys = es / nbx, exs = es - eys * nbx;
    if (abs(elox + exs - dxs) > c.fb || abs(eloy + eys - dys) > c.fb) o.status = kFbCheck;
  }
  if (o.status == kTracked) {
    // step 10: den >= 1 on both axes (the left and the upper neighbour of the smallest minimiser are strictly larger)
    const long long cmx = costs[ks - 1], cpx = costs[ks + 1], cmy = costs[ks - ncx], cpy = costs[ks + ncx];
    const long long denx = cmx + cpx - 2 * cost, deny = cmy + cpy - 2 * cost;
    const double deltax = (double)(cmx - cpx) / (double)(2 * denx), deltay = (double)(cmy - cpy) / (double)(2 * deny);
    o.x = __float_as_uint((float)(((double)x + (double)(xp - xa + dxs)) + deltax));
    o.y = __float_as_uint((float)(((double)y + (double)(yp - ya + dys)) + deltay));
  }
  return o;
}

}  // namespace search2d
}  // namespace patch_search
}  // namespace sship
