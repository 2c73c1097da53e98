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

#include <climits>
#include <cstdint>

#include "kernels.h"

namespace sship {

namespace {
constexpr int kLanes = kWave;                          // lanes per keypoint: one wave
constexpr int kSlots = 3;                              // keypoints per workgroup: 3 x 20 496 B = 61 488 B at half_window 7, search_radius 16
enum { kNone = 0, kTracked = 1, kBorder = 2, kRange = 3, kTexture = 4, kEdge = 5, kCost = 6, kAmbiguous = 7, kFbCheck = 8 };
constexpr uint32_t kQuietNan = 0x7fc00000u;

__host__ __device__ inline int round16(int v) { return (v + 15) & ~15; }
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
  for (int m = kLanes / 2; m >= 1; m >>= 1) {
    const long long oc = __shfl_xor(best, m, kLanes);
    const int ok = __shfl_xor(bk, m, kLanes);
    if (oc < best || (oc == best && ok < bk)) { best = oc; bk = ok; }
  }
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
  for (int k = t; k < nc; k += kLanes) {
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

// sum and sum of squares of the template over the wave (the padding is zero); every lane ends with the result
__device__ __forceinline__ void patch_sums(const uint8_t* patch, int bytes, int t, int& a1, int& a2) {
  a1 = 0; a2 = 0;
  for (int k = t; k < bytes; k += kLanes) { const int a = patch[k]; a1 += a; a2 += a * a; }
#pragma unroll
  for (int m = kLanes / 2; m >= 1; m >>= 1) { a1 += __shfl_xor(a1, m, kLanes); a2 += __shfl_xor(a2, m, kLanes); }
}

// hs / hq [r ncx + c] = the sum (of squares) of the pw region bytes of row r from column c on, r < rh, c < ncx: a lane per entry
__device__ __forceinline__ void row_sums(const uint8_t* region, int pw, int rw, int rh, int ncx, int t, uint32_t* hq, uint16_t* hs) {
  for (int k = t; k < rh * ncx; k += kLanes) {
    const int r = k / ncx, cc = k - r * ncx;
    const uint8_t* p = region + r * rw + cc;
    int s1 = 0, s2 = 0;
    for (int q = 0; q < pw; ++q) { const int v = p[q]; s1 += v; s2 += v * v; }
    hs[k] = (uint16_t)s1; hq[k] = (uint32_t)s2;          // <= 15 x 255 and 15 x 255^2
  }
}

// rh rows of rw bytes from src (row pitch `stride`) to dst (row pitch rw), the lanes side by side along the bytes of the region
__device__ __forceinline__ void stage_region(const uint8_t* __restrict__ src, long long stride, uint8_t* dst, int rh, int rw, int t) {
  for (int k = t; k < rh * rw; k += kLanes) {
    const int r = k / rw, cc = k - r * rw;
    dst[k] = src[r * stride + cc];
  }
}
// the template: pw rows of pw bytes from src to rows of `pitch` >= pw bytes, the rest of a row zero
__device__ __forceinline__ void stage_patch(const uint8_t* __restrict__ src, long long stride, uint8_t* dst, int pw, int pitch, int t) {
  for (int k = t; k < pw * pitch; k += kLanes) {
    const int r = k / pitch, cc = k % pitch;
    dst[k] = cc < pw ? src[r * stride + cc] : (uint8_t)0;
  }
}
}  // namespace

// pred and kp_out may be the same array (no __restrict__ on either): a wave reads its row of pred before lane 0 writes that row of kp_out,
// and no other wave touches the row
__global__ __launch_bounds__(kLanes * kSlots) void k_patch_track(const uint8_t* __restrict__ imgs0, long long image_stride0, long long stride0,
                                                                const uint8_t* __restrict__ imgs1, long long image_stride1, long long stride1,
                                                                int h, int w, const uint32_t* kp, const int* __restrict__ lens, int unit_stride,
                                                                const uint32_t* pred, int K, PatchTrackK c, uint32_t* kp_out, int* n_out,
                                                                int* matches_out, uint8_t* status_out, long long* cost_out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int pair = blockIdx.x, g = threadIdx.x / kLanes, t = threadIdx.x % kLanes;
  const int i = blockIdx.y * kSlots + g;
  if (i >= K) return;                                   // wave-uniform, and no workgroup barrier follows
  const int hw = c.half_window, R = c.radius, pw = 2 * hw + 1;
  const SlotLayout lay = slot_layout(hw, R);
  uint8_t* slot = smem + (size_t)g * lay.bytes;
  long long* costs = reinterpret_cast<long long*>(slot);
  uint8_t* patch = slot + lay.patch;
  uint8_t* region = slot + lay.region;
  uint32_t* hq = reinterpret_cast<uint32_t*>(slot + lay.hq);
  uint16_t* hs = reinterpret_cast<uint16_t*>(slot + lay.hs);
  const int pitch = 4 * ((pw + 3) / 4);                  // bytes of a template row in LDS
  ScanIn in{patch, region, hq, hs, pw, 0, 0, 0, 0};
  const size_t row = (size_t)pair * K + i, unit = (size_t)pair * unit_stride;

  uint32_t out_x = 0, out_y = 0, score = 0;
  int status = kNone, match = -1;
  long long cost = -1;
  const int n0 = min(max(lens[unit], 0), K);
  if (n_out && i == 0 && t == 0) n_out[pair] = n0;
  if (i < n0) {
    // step 2
    const uint32_t bx = kp[(unit * K + i) * 3], by = kp[(unit * K + i) * 3 + 1];
    score = kp[(unit * K + i) * 3 + 2];
    const float x = __uint_as_float(bx), y = __uint_as_float(by);
    const float px = pred ? __uint_as_float(pred[row * 3]) : x, py = pred ? __uint_as_float(pred[row * 3 + 1]) : y;
    out_x = kQuietNan; out_y = kQuietNan;
    status = kBorder;
    int xa = 0, ya = 0, xp = 0, yp = 0, lox = 0, loy = 0, ncx = 0, ncy = 0;
    if (coord_ok(x) && coord_ok(y) && coord_ok(px) && coord_ok(py)) {
      xa = (int)floor((double)x + 0.5); ya = (int)floor((double)y + 0.5);
      xp = (int)floor((double)px + 0.5); yp = (int)floor((double)py + 0.5);
      if (xa - hw >= 0 && xa + hw < w && ya - hw >= 0 && ya + hw < h) {
        // step 3: every candidate patch inside I1
        lox = max(-R, hw - xp); loy = max(-R, hw - yp);
        ncx = min(R, w - 1 - hw - xp) - lox + 1; ncy = min(R, h - 1 - hw - yp) - loy + 1;
        status = (ncx < 3 || ncy < 3) ? kRange : kTracked;
      }
    }
    if (status == kTracked) {
      // stage the template and the region of I1: byte (r, j) of the region is pixel (yp + loy - hw + r, xp + lox - hw + j), so candidate
      // (kx, ky) = (dx - lox, dy - loy) starts at row ky, column kx
      const uint8_t* i0 = imgs0 + (size_t)pair * image_stride0 + (size_t)(ya - hw) * stride0 + (xa - hw);
      const uint8_t* i1 = imgs1 + (size_t)pair * image_stride1 + (size_t)(yp + loy - hw) * stride1 + (xp + lox - hw);
      stage_patch(i0, stride0, patch, pw, pitch, t);
      stage_region(i1, stride1, region, ncy + pw - 1, ncx + pw - 1, t);
      wave_sync();
      patch_sums(patch, pw * pitch, t, in.a1, in.a2);
      // step 4
      if (c.tex) {
        const long long T = (long long)(pw * pw) * in.a2 - (long long)in.a1 * in.a1;
        if ((double)T < c.tex2) status = kTexture;
      }
    }
    if (status == kTracked) {
      // steps 5-8
      const int rw = ncx + pw - 1, rh = ncy + pw - 1, nc = ncx * ncy;
      long long best; int ks;
      row_sums(region, pw, rw, rh, ncx, t, hq, hs);
      wave_sync();
      in.rw = rw; in.ncx = ncx;
      scan_candidates(in, nc, 0, 0, 1, t, costs, best, ks);
      wave_argmin(best, ks);
      cost = best;
      wave_sync();                                      // the costs of the other lanes are read below
      const int kys = ks / ncx, kxs = ks - kys * ncx;
      const int dxs = lox + kxs, dys = loy + kys;
      if (kxs == 0 || kxs == ncx - 1 || kys == 0 || kys == ncy - 1) status = kEdge;
      else if (c.gate && (double)cost > c.gate2) status = kCost;
      else if (c.uniqueness > 0) {
        long long c2 = LLONG_MAX;
        for (int k = t; k < nc; k += kLanes) {
          const int ky = k / ncx, kx = k - ky * ncx;
          if (abs(kx - kxs) > 1 || abs(ky - kys) > 1) c2 = min(c2, costs[k]);
        }
#pragma unroll
        for (int m = kLanes / 2; m >= 1; m >>= 1) c2 = min(c2, (long long)__shfl_xor(c2, m, kLanes));
        if (c2 != LLONG_MAX && !(100 * cost < (long long)(100 - c.uniqueness) * c2)) status = kAmbiguous;
      }
      if (status == kTracked && c.fb >= 0) {
        // step 9: the I1 patch at the minimiser leaves the region for the template buffer; the region of I0 that holds the patches at
        // (cx - ex, cy - ey) takes its place, column 0 at cx - ehix - hw: candidate (kx, ky) = (ex - elox, ey - eloy) starts at row
        // nby - 1 - ky, column nbx - 1 - kx
        const int cx = xa + dxs, cy = ya + dys;
        const int elox = max(-R, cx - (w - 1 - hw)), ehix = min(R, cx - hw), eloy = max(-R, cy - (h - 1 - hw)), ehiy = min(R, cy - hw);
        const int nbx = ehix - elox + 1, nby = ehiy - eloy + 1, rw2 = nbx + pw - 1, rh2 = nby + pw - 1;
        uint8_t keep[4];                                // pw^2 <= 225 < 4 * 64
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = t + q * kLanes;
          keep[q] = k < pw * pw ? region[(kys + k / pw) * rw + kxs + k % pw] : 0;
        }
        wave_sync();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = t + q * kLanes;
          if (k < pw * pw) patch[(k / pw) * pitch + k % pw] = keep[q];   // the padding stays zero
        }
        const uint8_t* i0 = imgs0 + (size_t)pair * image_stride0 + (size_t)(cy - ehiy - hw) * stride0 + (cx - ehix - hw);
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
        if (abs(elox + exs - dxs) > c.fb || abs(eloy + eys - dys) > c.fb) status = kFbCheck;
      }
      if (status == kTracked) {
        // step 10: den >= 1 on both axes (the left and the upper neighbour of the smallest minimiser are strictly larger)
        const long long cmx = costs[ks - 1], cpx = costs[ks + 1], cmy = costs[ks - ncx], cpy = costs[ks + ncx];
        const long long denx = cmx + cpx - 2 * cost, deny = cmy + cpy - 2 * cost;
        const double deltax = (double)(cmx - cpx) / (double)(2 * denx), deltay = (double)(cmy - cpy) / (double)(2 * deny);
        out_x = __float_as_uint((float)(((double)x + (double)(xp - xa + dxs)) + deltax));
        out_y = __float_as_uint((float)(((double)y + (double)(yp - ya + dys)) + deltay));
        match = i;
      }
    }
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
