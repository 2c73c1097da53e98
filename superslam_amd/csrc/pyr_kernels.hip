// Image pyramid and coarse-to-fine patch tracking (include/sship.h "Image pyramid" and "Coarse-to-fine patch tracking").
//   k_pyr_down<ALIGNED>  one reduction (5 x 5 binomial, reflect-101 borders, every second pixel): a 256-thread workgroup owns a 64 x 16
//                        output tile of one image, one launch per level for the whole batch.
//   k_pyr_track          the 2-D patch search (patch_search.h) walked down the levels by the wave that owns the keypoint: one wave per
//                        keypoint, 3 keypoints per 192-thread workgroup, one launch for the whole call.
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
// k_pyr_track calls the per-keypoint body that k_patch_track runs once (patch_search.h's track_level: its LDS slot, its scan on packed
// bytes, its butterflies) once per level, from the top down.  Keypoints are independent, so the prediction a level hands to the next
// one lives in the wave's registers; nothing but the call's outputs reaches memory.  The per-level pointers, strides and sizes arrive by
// value.  The slot is sized on the host for max(fine.search_radius, coarse_radius); a level lays its own (smaller or equal) layout over it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "patch_search.h"

namespace sship {

using namespace patch_search;
using namespace patch_search::search2d;

namespace {
constexpr int kLanes = kWave;                          // the tracker's lanes per keypoint: one wave
constexpr int kSlots = 3;                              // its keypoints per workgroup: 3 x 20 496 B = 61 488 B at half_window 7, radius 16

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
// the tracker
// ------------------------------------------------------------------------------------------------------
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
      wave_sync();                                      // the level above read its costs: this level's staging lies over them
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
