// Image pyramid and coarse-to-fine patch tracking (include/sship.h "Image pyramid" and "Coarse-to-fine patch tracking").
//   k_pyr_down<ALIGNED>  one reduction (5 x 5 binomial, reflect-101 borders, every second pixel): a 256-thread workgroup owns a 64 x 16
//                        output tile of one image, one launch per level for the whole batch.
//   k_pyr_track          the patch search of patch_track_kernels.hip walked down the levels by the wave that owns the keypoint: one wave
//                        per keypoint, 3 keypoints per 192-thread workgroup, one launch for the whole call.
//
// k_pyr_down stages the 35 rows x 136 bytes of the source that its tile needs (source columns 128 tx - 4 .. 128 tx + 131, rows 32 ty - 2 ..
// 32 ty + 32, every index through reflect-101, so no load leaves the image) as dwords in LDS: with byte loads where nothing is known about
// the rows (the caller's level 0 at an odd pointer or stride), with one dword load wherever the four columns lie inside the row where every
// row starts on a multiple of 4 bytes (the handle's own levels, whose rows start on 64 bytes, and a level 0 that happens to be so: the host
// picks the instantiation per launch).  The horizontal pass turns three LDS dwords into two 16-bit sums (<= 16 x 255), packed in one dword; the
// vertical pass adds five of those dwords with the weights 1 4 6 4 1 - both halves stay below 2^16 (65 280 + 128), so the two columns never
// meet - and a thread stores the four pixels of its dword whole into the padded row (bytes past the level's width are zero).  9 240 B of
// static LDS, no scratch.
//
// k_pyr_track keeps k_patch_track's per-keypoint body (its LDS slot, its scan on packed bytes, its butterflies; see that file) as one
// device function and calls it once per level, from the top down.  Keypoints are independent, so the prediction a level hands to the next
// one lives in the wave's registers; nothing but the call's outputs reaches memory.  The per-level pointers, strides and sizes arrive by
// value.  The slot is sized on the host for max(fine.search_radius, coarse_radius); a level lays its own (smaller or equal) layout over it.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "kernels.h"

namespace sship {

namespace {
// ------------------------------------------------------------------------------------------------------
// the reduction
// ------------------------------------------------------------------------------------------------------
constexpr int kBoxRows = 2 * kPyrTileH + 3;            // 35 source rows per tile
constexpr int kBoxDwords = (2 * kPyrTileW + 8) / 4;    // 34 dwords per staged row: source columns 128 tx - 4 .. 128 tx + 131
constexpr int kHorDwords = kPyrTileW / 2;              // 32 pairs of 16-bit horizontal sums per row

// reflect-101 applied until the index is inside: the map has period 2 (n - 1)
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}
}  // namespace

template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_pyr_down(const uint8_t* __restrict__ src, long long src_image_stride, long long src_stride, int h, int w,
                                                  uint8_t* __restrict__ dst, long long dst_image_stride, int dst_pitch, int tiles_x) {
  __shared__ uint32_t box[kBoxRows * kBoxDwords];
  __shared__ uint32_t hor[kBoxRows * kHorDwords];
  const int tid = threadIdx.x, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int X0 = 2 * kPyrTileW * tx - 4, Y0 = 2 * kPyrTileH * ty - 2;
  const uint8_t* s = src + (size_t)blockIdx.y * src_image_stride;
  for (int k = tid; k < kBoxRows * kBoxDwords; k += 256) {
    const int r = k / kBoxDwords, d = k - r * kBoxDwords;
    const uint8_t* row = s + (size_t)reflect101(Y0 + r, h) * src_stride;
    const int X = X0 + 4 * d;
    uint32_t v;
    if (X >= 0 && X + 3 < w) {
      if (ALIGNED) v = *reinterpret_cast<const uint32_t*>(row + X);   // every row starts on a multiple of 4 bytes, and X is one
      else v = (uint32_t)row[X] | (uint32_t)row[X + 1] << 8 | (uint32_t)row[X + 2] << 16 | (uint32_t)row[X + 3] << 24;
    } else {
      v = (uint32_t)row[reflect101(X, w)] | (uint32_t)row[reflect101(X + 1, w)] << 8 | (uint32_t)row[reflect101(X + 2, w)] << 16 |
          (uint32_t)row[reflect101(X + 3, w)] << 24;
    }
    box[k] = v;
  }
  __syncthreads();
  // outputs x = 2 q and 2 q + 1 of the tile read staged bytes 4 q + 2 .. 4 q + 8 (the centre of output x is staged byte 2 x + 4)
  for (int k = tid; k < kBoxRows * kHorDwords; k += 256) {
    const int r = k / kHorDwords, q = k - r * kHorDwords;
    const uint32_t w0 = box[r * kBoxDwords + q], w1 = box[r * kBoxDwords + q + 1], w2 = box[r * kBoxDwords + q + 2];
    const uint32_t b2 = (w0 >> 16) & 255u, b3 = w0 >> 24, b4 = w1 & 255u, b5 = (w1 >> 8) & 255u, b6 = (w1 >> 16) & 255u, b7 = w1 >> 24, b8 = w2 & 255u;
    const uint32_t lo = b2 + 4u * b3 + 6u * b4 + 4u * b5 + b6, hi = b4 + 4u * b5 + 6u * b6 + 4u * b7 + b8;
    hor[k] = lo | hi << 16;
  }
  __syncthreads();
  const int oy = tid / 16, dq = tid % 16;
  const int h2 = (h + 1) / 2, w2 = (w + 1) / 2, gy = kPyrTileH * ty + oy, gx = kPyrTileW * tx + 4 * dq;
  if (gy >= h2 || gx >= w2) return;
  uint32_t out = 0;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const uint32_t* p = hor + (2 * oy) * kHorDwords + 2 * dq + half;
    // two 16-bit columns per dword: each stays <= 65 280 + 128
    const uint32_t acc = p[0] + 4u * p[kHorDwords] + 6u * p[2 * kHorDwords] + 4u * p[3 * kHorDwords] + p[4 * kHorDwords] + 0x00800080u;
    out |= (((acc >> 8) & 255u) | ((acc >> 24) << 8)) << (16 * half);
  }
  const int left = w2 - gx;                             // the pixels of this dword inside the level: the padding is zero
  if (left < 4) out &= (1u << (8 * left)) - 1u;
  *reinterpret_cast<uint32_t*>(dst + (size_t)blockIdx.y * dst_image_stride + (size_t)gy * dst_pitch + gx) = out;
}

void launch_pyr_down(const uint8_t* src, long long src_image_stride, long long src_stride, int h, int w, int aligned, uint8_t* dst,
                     long long dst_image_stride, int dst_pitch, int images, hipStream_t s) {
  const int tiles_x = ((w + 1) / 2 + kPyrTileW - 1) / kPyrTileW, tiles_y = ((h + 1) / 2 + kPyrTileH - 1) / kPyrTileH;
  const dim3 grid(tiles_x * tiles_y, images);
  if (aligned)
    hipLaunchKernelGGL(k_pyr_down<true>, grid, dim3(256), 0, s, src, src_image_stride, src_stride, h, w, dst, dst_image_stride, dst_pitch, tiles_x);
  else
    hipLaunchKernelGGL(k_pyr_down<false>, grid, dim3(256), 0, s, src, src_image_stride, src_stride, h, w, dst, dst_image_stride, dst_pitch, tiles_x);
}

// ------------------------------------------------------------------------------------------------------
// the tracker: k_patch_track's helpers and per-keypoint body (patch_track_kernels.hip explains them), the body as a function of one level
// ------------------------------------------------------------------------------------------------------
namespace {
constexpr int kLanes = kWave;                          // lanes per keypoint: one wave
constexpr int kSlots = 3;                              // keypoints per workgroup: 3 x 20 496 B = 61 488 B at half_window 7, radius 16
enum { kNone = 0, kTracked = 1, kBorder = 2, kRange = 3, kTexture = 4, kEdge = 5, kCost = 6, kAmbiguous = 7, kFbCheck = 8 };
constexpr uint32_t kQuietNan = 0x7fc00000u;

__host__ __device__ inline int round16(int v) { return (v + 15) & ~15; }
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

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void wave_argmin(long long& best, int& bk) {
#pragma unroll
  for (int m = kLanes / 2; m >= 1; m >>= 1) {
    const long long oc = __shfl_xor(best, m, kLanes);
    const int ok = __shfl_xor(bk, m, kLanes);
    if (oc < best || (oc == best && ok < bk)) { best = oc; bk = ok; }
  }
}

struct ScanIn { const uint8_t* patch; const uint8_t* region; const uint32_t* hq; const uint16_t* hs; int pw, rw, ncx, a1, a2; };

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
        cross = __builtin_amdgcn_udot4(a[q], __builtin_amdgcn_alignbyte(w1, w0, sh), cross, false);
        w0 = w1;
      }
    }
    const int s1 = in.a1 - r1, s2 = in.a2 + r2 - 2 * (int)cross;
    const long long c = N * s2 - (long long)s1 * s1;
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

__device__ __forceinline__ void patch_sums(const uint8_t* patch, int bytes, int t, int& a1, int& a2) {
  a1 = 0; a2 = 0;
  for (int k = t; k < bytes; k += kLanes) { const int a = patch[k]; a1 += a; a2 += a * a; }
#pragma unroll
  for (int m = kLanes / 2; m >= 1; m >>= 1) { a1 += __shfl_xor(a1, m, kLanes); a2 += __shfl_xor(a2, m, kLanes); }
}

__device__ __forceinline__ void row_sums(const uint8_t* region, int pw, int rw, int rh, int ncx, int t, uint32_t* hq, uint16_t* hs) {
  for (int k = t; k < rh * ncx; k += kLanes) {
    const int r = k / ncx, cc = k - r * ncx;
    const uint8_t* p = region + r * rw + cc;
    int s1 = 0, s2 = 0;
    for (int q = 0; q < pw; ++q) { const int v = p[q]; s1 += v; s2 += v * v; }
    hs[k] = (uint16_t)s1; hq[k] = (uint32_t)s2;
  }
}

__device__ __forceinline__ void stage_region(const uint8_t* __restrict__ src, long long stride, uint8_t* dst, int rh, int rw, int t) {
  for (int k = t; k < rh * rw; k += kLanes) {
    const int r = k / rw, cc = k - r * rw;
    dst[k] = src[r * stride + cc];
  }
}
__device__ __forceinline__ void stage_patch(const uint8_t* __restrict__ src, long long stride, uint8_t* dst, int pw, int pitch, int t) {
  for (int k = t; k < pw * pitch; k += kLanes) {
    const int r = k / pitch, cc = k % pitch;
    dst[k] = cc < pw ? src[r * stride + cc] : (uint8_t)0;
  }
}

struct LevelOut { int status; long long cost; uint32_t x, y; };   // x, y: the bits of (x', y'), quiet NaNs unless the status is TRACKED

// steps 2 to 10 of the patch-tracking rule for one keypoint inside the count, on the images (i0, i1) of h x w pixels, by one wave.  Every
// lane returns the same values.  The template is read only after step 2 found it inside I0, the region only after step 3 found a box of at
// least 3 x 3 candidates whose patches lie inside I1: no load leaves an image.
__device__ __forceinline__ LevelOut track_level(const uint8_t* __restrict__ i0p, long long stride0, const uint8_t* __restrict__ i1p, long long stride1,
                                                int h, int w, float x, float y, float px, float py, const PatchTrackK& c, uint8_t* slot, int t) {
  const int hw = c.half_window, R = c.radius, pw = 2 * hw + 1;
  const SlotLayout lay = slot_layout(hw, R);
  long long* costs = reinterpret_cast<long long*>(slot);
  uint8_t* patch = slot + lay.patch;
  uint8_t* region = slot + lay.region;
  uint32_t* hq = reinterpret_cast<uint32_t*>(slot + lay.hq);
  uint16_t* hs = reinterpret_cast<uint16_t*>(slot + lay.hs);
  const int pitch = 4 * ((pw + 3) / 4);
  ScanIn in{patch, region, hq, hs, pw, 0, 0, 0, 0};
  LevelOut o{kBorder, -1, kQuietNan, kQuietNan};
  int xa = 0, ya = 0, xp = 0, yp = 0, lox = 0, loy = 0, ncx = 0, ncy = 0;
  wave_sync();                                          // the level above read its costs: this level's staging lies over them
  if (coord_ok(x) && coord_ok(y) && coord_ok(px) && coord_ok(py)) {
    xa = (int)floor((double)x + 0.5); ya = (int)floor((double)y + 0.5);
    xp = (int)floor((double)px + 0.5); yp = (int)floor((double)py + 0.5);
    if (xa - hw >= 0 && xa + hw < w && ya - hw >= 0 && ya + hw < h) {
      lox = max(-R, hw - xp); loy = max(-R, hw - yp);
      ncx = min(R, w - 1 - hw - xp) - lox + 1; ncy = min(R, h - 1 - hw - yp) - loy + 1;
      o.status = (ncx < 3 || ncy < 3) ? kRange : kTracked;
    }
  }
  if (o.status == kTracked) {
    const uint8_t* i0 = i0p + (size_t)(ya - hw) * stride0 + (xa - hw);
    const uint8_t* i1 = i1p + (size_t)(yp + loy - hw) * stride1 + (xp + lox - hw);
    stage_patch(i0, stride0, patch, pw, pitch, t);
    stage_region(i1, stride1, region, ncy + pw - 1, ncx + pw - 1, t);
    wave_sync();
    patch_sums(patch, pw * pitch, t, in.a1, in.a2);
    if (c.tex) {
      const long long T = (long long)(pw * pw) * in.a2 - (long long)in.a1 * in.a1;
      if ((double)T < c.tex2) o.status = kTexture;
    }
  }
  if (o.status != kTracked) return o;
  const int rw = ncx + pw - 1, rh = ncy + pw - 1, nc = ncx * ncy;
  long long best; int ks;
  row_sums(region, pw, rw, rh, ncx, t, hq, hs);
  wave_sync();
  in.rw = rw; in.ncx = ncx;
  scan_candidates(in, nc, 0, 0, 1, t, costs, best, ks);
  wave_argmin(best, ks);
  const long long cost = best;
  o.cost = cost;
  wave_sync();
  const int kys = ks / ncx, kxs = ks - kys * ncx;
  const int dxs = lox + kxs, dys = loy + kys;
  if (kxs == 0 || kxs == ncx - 1 || kys == 0 || kys == ncy - 1) o.status = kEdge;
  else if (c.gate && (double)cost > c.gate2) o.status = kCost;
  else if (c.uniqueness > 0) {
    long long c2 = LLONG_MAX;
    for (int k = t; k < nc; k += kLanes) {
      const int ky = k / ncx, kx = k - ky * ncx;
      if (abs(kx - kxs) > 1 || abs(ky - kys) > 1) c2 = min(c2, costs[k]);
    }
#pragma unroll
    for (int m = kLanes / 2; m >= 1; m >>= 1) c2 = min(c2, (long long)__shfl_xor(c2, m, kLanes));
    if (c2 != LLONG_MAX && !(100 * cost < (long long)(100 - c.uniqueness) * c2)) o.status = kAmbiguous;
  }
  if (o.status == kTracked && c.fb >= 0) {
    const int cx = xa + dxs, cy = ya + dys;
    const int elox = max(-R, cx - (w - 1 - hw)), ehix = min(R, cx - hw), eloy = max(-R, cy - (h - 1 - hw)), ehiy = min(R, cy - hw);
    const int nbx = ehix - elox + 1, nby = ehiy - eloy + 1, rw2 = nbx + pw - 1, rh2 = nby + pw - 1;
    uint8_t keep[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = t + q * kLanes;
      keep[q] = k < pw * pw ? region[(kys + k / pw) * rw + kxs + k % pw] : 0;
    }
    wave_sync();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = t + q * kLanes;
      if (k < pw * pw) patch[(k / pw) * pitch + k % pw] = keep[q];
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
    const long long cmx = costs[ks - 1], cpx = costs[ks + 1], cmy = costs[ks - ncx], cpy = costs[ks + ncx];
    const long long denx = cmx + cpx - 2 * cost, deny = cmy + cpy - 2 * cost;
    const double deltax = (double)(cmx - cpx) / (double)(2 * denx), deltay = (double)(cmy - cpy) / (double)(2 * deny);
    o.x = __float_as_uint((float)(((double)x + (double)(xp - xa + dxs)) + deltax));
    o.y = __float_as_uint((float)(((double)y + (double)(yp - ya + dys)) + deltay));
  }
  return o;
}
}  // namespace

// pred and kp_out may be the same array: a wave reads its row of pred before lane 0 writes that row of kp_out, and no other wave touches it
__global__ __launch_bounds__(kLanes * kSlots) void k_pyr_track(PyrTrackLevels tab, const uint32_t* kp, const int* __restrict__ lens, int unit_stride,
                                                              const uint32_t* pred, int K, PyrTrackK c, uint32_t* kp_out, int* n_out,
                                                              int* matches_out, uint8_t* status_out, long long* cost_out, uint8_t* levels_out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int pair = blockIdx.x, g = threadIdx.x / kLanes, t = threadIdx.x % kLanes;
  const int i = blockIdx.y * kSlots + g;
  if (i >= K) return;                                   // wave-uniform, and no workgroup barrier follows
  uint8_t* slot = smem + (size_t)g * c.slot_bytes;
  const size_t row = (size_t)pair * K + i, unit = (size_t)pair * unit_stride;

  uint32_t out_x = 0, out_y = 0, score = 0;
  int status = kNone, match = -1, mask = 0;
  long long cost = -1;
  const int n0 = min(max(lens[unit], 0), K);
  if (n_out && i == 0 && t == 0) n_out[pair] = n0;
  if (i < n0) {
    const float x = __uint_as_float(kp[(unit * K + i) * 3]), y = __uint_as_float(kp[(unit * K + i) * 3 + 1]);
    score = kp[(unit * K + i) * 3 + 2];
    const int top = c.levels - 1;
    const double st = 1.0 / (double)(1 << top);
    // the top level's prediction: one rounding of the fp64 product
    float px = (float)((double)(pred ? __uint_as_float(pred[row * 3]) : x) * st);
    float py = (float)((double)(pred ? __uint_as_float(pred[row * 3 + 1]) : y) * st);
    PatchTrackK coarse = c.fine;
    coarse.radius = c.coarse_radius; coarse.tex = 0; coarse.gate = 0; coarse.fb = -1;
    for (int l = top; l >= 0; --l) {
      const PyrTrackLevel& L = tab.l[l];
      const double sl = 1.0 / (double)(1 << l);
      const float xl = (float)((double)x * sl), yl = (float)((double)y * sl);
      const LevelOut o = track_level(L.img0 + (size_t)pair * L.pair_stride0, L.stride0, L.img1 + (size_t)pair * L.pair_stride1, L.stride1, L.h, L.w,
                                     xl, yl, px, py, l ? coarse : c.fine, slot, t);
      if (o.status == kTracked) mask |= 1 << l;
      if (l) {                                          // exact doublings
        px = 2.f * (o.status == kTracked ? __uint_as_float(o.x) : px);
        py = 2.f * (o.status == kTracked ? __uint_as_float(o.y) : py);
      } else {
        status = o.status; cost = o.cost; out_x = o.x; out_y = o.y;
        if (status == kTracked) match = i;
      }
    }
  }
  if (t != 0) return;
  kp_out[row * 3] = out_x; kp_out[row * 3 + 1] = out_y; kp_out[row * 3 + 2] = score;
  matches_out[row] = match;
  if (status_out) status_out[row] = (uint8_t)status;
  if (cost_out) cost_out[row] = cost;
  if (levels_out) levels_out[row] = (uint8_t)mask;
}

size_t pyr_track_slot_bytes(int half_window, int radius) { return (size_t)slot_layout(half_window, radius).bytes; }

void launch_pyr_track(const PyrTrackLevels& tab, int pairs, const float* kp, const int* lens, int unit_stride, const float* pred, int max_kp,
                      const PyrTrackK& c, float* kp_out, int* n_out, int* matches0, uint8_t* status, long long* cost, uint8_t* levels_tracked,
                      hipStream_t s) {
  const size_t smem = (size_t)kSlots * c.slot_bytes;    // 61 488 B at the largest parameters
  hipLaunchKernelGGL(k_pyr_track, dim3(pairs, (max_kp + kSlots - 1) / kSlots), dim3(kLanes * kSlots), smem, s, tab,
                     reinterpret_cast<const uint32_t*>(kp), lens, unit_stride, reinterpret_cast<const uint32_t*>(pred), max_kp, c,
                     reinterpret_cast<uint32_t*>(kp_out), n_out, matches0, status, cost, levels_tracked);
}

}  // namespace sship
