// FAST corners with track refill (include/sship.h "FAST corners").
//   k_fast_score<ALIGNED>         the stage form of step 1: one 256-thread workgroup writes the u8 scores of a 64 x 32 tile of one image.
//   k_fast_detect<ALIGNED, MASK>  steps 1-3: one 256-thread workgroup owns a 64 x 32 tile of one image, grid (tiles, images).
//   k_fast_merge                  step 5: one 1024-thread workgroup per image.
// Step 4 is k_topk / k_select_balanced of sp_kernels.hip, unchanged, on the key list k_fast_detect leaves.
//
// Both tile kernels stage the tile plus a 4-pixel halo (3 for the ring, 1 for the non-maximum test) in LDS, 40 rows of 72 bytes, zeros
// outside the image.  The tile's first staged column is a multiple of 4 pixels, so with ALIGNED (pointer, image stride and row stride
// multiples of 4, picked on the host per launch) a dword that lies whole inside the image is one load; every other unit, and every unit
// without ALIGNED, goes byte by byte and never outside [0, w) x [0, h).  The score of a pixel is formed from the 16 ring differences in
// registers: the minimum (maximum) over every circular window of 9 by doubling - windows of 2, 4, 8, then 8 + 1 - which is 4 x 16
// min and 4 x 16 max in place of 2 x 16 x 8, and exact: integers throughout.  bright = max_a min9_a, dark = -min_a max9_a.
// k_fast_detect needs s only where s > t: a pixel with s <= t is no candidate and loses every comparison against one, whatever value
// stands for it, so it is written as 0.  An arc of 9 holds at least one pixel of every opposite pair (k, k + 8), so s > t needs
// max(e_k, e_k+8) > t for every pair (bright) or min(e_k, e_k+8) < -t for every pair (dark).  Pass 1 tests that on the two pairs of
// the compass ring pixels (5 LDS bytes) for every pixel of the tile plus one (66 x 34) and compacts the positions that pass
// into an LDS list; pass 2 scores the listed positions exactly, lanes dense.  Then a thread tests 8 tile pixels: s > t, inside the border,
// (s, y, x) greater than that of the 8 neighbours (>= against the 4 earlier in raster order, > against the 4 later), mask bit clear.
// The mask (MASK: keep given and d > 0) is built per tile in LDS, one 64-bit word per tile row: a thread takes keep rows i, i + 256, ...,
// clips the box of a live row to the tile and ORs its columns into the rows it covers (LDS atomics; OR commutes, so the mask does not
// depend on their order).  Survivors go to an LDS list through one LDS atomic per wave; the workgroup reserves its slots in the image's
// key list with ONE global atomic (as k_nms_tile does) and copies the keys.  No two candidates are 8-neighbours, so a tile holds at most
// 32 x 16 = 512 and an image at most ceil(h/2) * ceil(w/2): the host sizes the list to that, it cannot overflow, and the order the
// reservations resolve in changes the list's order only, which the selection does not see (it sorts distinct keys).  No scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace sship {

namespace {
constexpr int kThreads = 256;
constexpr int kTW = kFastTileW, kTH = kFastTileH, kHalo = 4;
constexpr int kPW = kTW + 2 * kHalo, kPH = kTH + 2 * kHalo;   // staged pixels: 72 x 40
constexpr int kSW = kTW + 2, kSH = kTH + 2, kSP = 68;         // scored pixels: 66 x 34 in rows of 68 bytes
constexpr int kTileCand = (kTW / 2) * (kTH / 2);
static_assert(kPW % 4 == 0 && kTW % 4 == 0, "the staged row starts on a dword of the image row");

__device__ __forceinline__ bool fast_coord_ok(float x) { return x >= 0.f && x < 16384.f; }   // NaN and +-inf: false

// the tile at (X0, Y0) plus its halo into pix[kPH][kPW]
template <bool ALIGNED>
__device__ __forceinline__ void stage_tile(const uint8_t* __restrict__ img, long long stride, int h, int w, int X0, int Y0, uint8_t* pix) {
  uint32_t* pix32 = reinterpret_cast<uint32_t*>(pix);
  for (int k = threadIdx.x; k < kPH * (kPW / 4); k += kThreads) {
    const int r = k / (kPW / 4), q = k - r * (kPW / 4);
    const int y = Y0 - kHalo + r, x = X0 - kHalo + 4 * q;
    uint32_t v = 0;
    if (y >= 0 && y < h && x + 3 >= 0 && x < w) {
      const uint8_t* row = img + (size_t)y * stride;
      if (ALIGNED && x >= 0 && x + 3 < w) {
        v = *reinterpret_cast<const uint32_t*>(row + x);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (x + b >= 0 && x + b < w) v |= (uint32_t)row[x + b] << (8 * b);
      }
    }
    pix32[k] = v;
  }
}

// step 1 at staged position (px, py): the caller has checked that the ring lies inside the image
__device__ __forceinline__ int fast_score_at(const uint8_t* pix, int px, int py) {
  const uint8_t* c = pix + py * kPW + px;
  const int v = c[0];
  int e[16];
  e[0] = c[-3 * kPW] - v;      e[1] = c[-3 * kPW + 1] - v;  e[2] = c[-2 * kPW + 2] - v;  e[3] = c[-kPW + 3] - v;
  e[4] = c[3] - v;             e[5] = c[kPW + 3] - v;       e[6] = c[2 * kPW + 2] - v;   e[7] = c[3 * kPW + 1] - v;
  e[8] = c[3 * kPW] - v;       e[9] = c[3 * kPW - 1] - v;   e[10] = c[2 * kPW - 2] - v;  e[11] = c[kPW - 3] - v;
  e[12] = c[-3] - v;           e[13] = c[-kPW - 3] - v;     e[14] = c[-2 * kPW - 2] - v; e[15] = c[-3 * kPW - 1] - v;
  int lo2[16], hi2[16], lo4[16], hi4[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) { lo2[k] = min(e[k], e[(k + 1) & 15]); hi2[k] = max(e[k], e[(k + 1) & 15]); }
#pragma unroll
  for (int k = 0; k < 16; ++k) { lo4[k] = min(lo2[k], lo2[(k + 2) & 15]); hi4[k] = max(hi2[k], hi2[(k + 2) & 15]); }
  int bright = -255, dark_neg = 255;   // max over arcs of the arc's minimum; min over arcs of the arc's maximum
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int lo9 = min(min(lo4[k], lo4[(k + 4) & 15]), e[(k + 8) & 15]);
    const int hi9 = max(max(hi4[k], hi4[(k + 4) & 15]), e[(k + 8) & 15]);
    bright = max(bright, lo9);
    dark_neg = min(dark_neg, hi9);
  }
  return max(max(bright, -dark_neg), 0);
}

__device__ __forceinline__ bool ring_inside(int x, int y, int h, int w) { return x >= 3 && x < w - 3 && y >= 3 && y < h - 3; }
}  // namespace

template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_fast_score(const uint8_t* __restrict__ imgs, long long image_stride, long long stride, int h, int w,
                                                    int tiles_x, uint8_t* __restrict__ score, long long score_image_stride,
                                                    long long score_stride) {
  __shared__ __attribute__((aligned(16))) uint8_t pix[kPH * kPW];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int X0 = tx * kTW, Y0 = ty * kTH;
  stage_tile<ALIGNED>(imgs + (size_t)blockIdx.y * image_stride, stride, h, w, X0, Y0, pix);
  __syncthreads();
  uint8_t* out = score + (size_t)blockIdx.y * score_image_stride;
  for (int k = threadIdx.x; k < kTW * kTH; k += kThreads) {
    const int r = k / kTW, c = k - r * kTW, x = X0 + c, y = Y0 + r;
    if (x >= w || y >= h) continue;
    out[(size_t)y * score_stride + x] = ring_inside(x, y, h, w) ? (uint8_t)fast_score_at(pix, c + kHalo, r + kHalo) : (uint8_t)0;
  }
}

namespace {
// Necessary for s > t at staged position (px, py): every opposite pair of the ring holds a pixel brighter than the centre by more than t,
// or every pair one darker by more than t; tested on the pairs (0, 8) and (4, 12).  (On the benchmark's synthetic frames at t = 20, 1.27 %
// of the pixels pass these two pairs, 1.06 % four pairs and 1.00 % all eight; 0.60 % have s > t.)
__device__ __forceinline__ bool fast_may_exceed(const uint8_t* pix, int px, int py, int t) {
  const uint8_t* c = pix + py * kPW + px;
  const int v = c[0];
  const int e0 = c[-3 * kPW] - v, e8 = c[3 * kPW] - v, e4 = c[3] - v, e12 = c[-3] - v;
  return min(max(e0, e8), max(e4, e12)) > t || max(min(e0, e8), min(e4, e12)) < -t;
}
}  // namespace

template <bool ALIGNED, bool MASK>
__global__ __launch_bounds__(256) void k_fast_detect(const uint8_t* __restrict__ imgs, long long image_stride, long long stride, FastK c,
                                                     const float* __restrict__ keep, const int* __restrict__ keep_n,
                                                     unsigned long long* __restrict__ cand, int* __restrict__ cand_count) {
  __shared__ __attribute__((aligned(16))) uint8_t pix[kPH * kPW];
  __shared__ __attribute__((aligned(16))) uint8_t sc[kSH * kSP];
  __shared__ unsigned long long keys[kTileCand];
  __shared__ unsigned long long tmask[kTH];        // bit q of row r: tile pixel (X0 + q, Y0 + r) lies within d of a live keep row
  __shared__ unsigned short todo[kSW * kSH];       // the scored positions (r * kSW + q) that passed the quick test
  __shared__ int s_todo, s_cnt, s_base;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int ty = blockIdx.x / c.tiles_x, tx = blockIdx.x - ty * c.tiles_x;
  const int X0 = tx * kTW, Y0 = ty * kTH, h = c.h, w = c.w;
  if (tid == 0) { s_cnt = 0; s_todo = 0; }
  if (MASK && tid < kTH) tmask[tid] = 0ull;
  stage_tile<ALIGNED>(imgs + (size_t)blockIdx.y * image_stride, stride, h, w, X0, Y0, pix);
  __syncthreads();
  if (MASK) {
    const int d = c.min_distance;
    const size_t unit = (size_t)blockIdx.y * c.unit_stride;
    const int n_keep = min(max(keep_n[unit], 0), c.max_kp);
    const float* rows = keep + unit * c.max_kp * 3;
    for (int i = tid; i < n_keep; i += kThreads) {
      const float x = rows[3 * i], y = rows[3 * i + 1];
      if (!fast_coord_ok(x) || !fast_coord_ok(y)) continue;
      const int xa = (int)floor((double)x + 0.5), ya = (int)floor((double)y + 0.5);
      const int q0 = max(xa - d + 1 - X0, 0), q1 = min(xa + d - 1 - X0, kTW - 1);
      const int r0 = max(ya - d + 1 - Y0, 0), r1 = min(ya + d - 1 - Y0, kTH - 1);
      if (q0 > q1 || r0 > r1) continue;
      const unsigned long long bits = (q1 == 63 ? ~0ull : ((1ull << (q1 + 1)) - 1ull)) & ~((1ull << q0) - 1ull);
      for (int r = r0; r <= r1; ++r) atomicOr(&tmask[r], bits);
    }
  }
  // pass 1: the quick test on every position of the tile plus one; every lane of a wave stays in the loop for the ballot
  for (int k0 = 0; k0 < kSW * kSH; k0 += kThreads) {
    const int k = k0 + tid;
    bool pass = false;
    if (k < kSW * kSH) {
      const int r = k / kSW, q = k - r * kSW;
      sc[r * kSP + q] = 0;
      pass = ring_inside(X0 - 1 + q, Y0 - 1 + r, h, w) && fast_may_exceed(pix, q + kHalo - 1, r + kHalo - 1, c.threshold);
    }
    const unsigned long long act = __ballot(pass);
    if (act) {
      const int leader = __ffsll((long long)act) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(&s_todo, __popcll(act));
      base = __shfl(base, leader, kWave);
      if (pass) todo[base + __popcll(act & ((1ull << lane) - 1ull))] = (unsigned short)k;   // at most kSW * kSH positions pass
    }
  }
  __syncthreads();
  // pass 2: the exact score of the listed positions
  const int n_todo = min(s_todo, kSW * kSH);
  for (int i = tid; i < n_todo; i += kThreads) {
    const int k = todo[i], r = k / kSW, q = k - r * kSW;
    sc[r * kSP + q] = (uint8_t)fast_score_at(pix, q + kHalo - 1, r + kHalo - 1);
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < kTW * kTH / kThreads; ++p) {
    const int k = tid + p * kThreads;
    const int r = k / kTW, q = k - r * kTW, x = X0 + q, y = Y0 + r;
    const uint8_t* m = sc + (r + 1) * kSP + (q + 1);
    const int s = m[0];
    bool take = s > c.threshold && x >= c.border && x < w - c.border && y >= c.border && y < h - c.border;
    if (take) {
      const int before = max(max((int)m[-kSP - 1], (int)m[-kSP]), max((int)m[-kSP + 1], (int)m[-1]));   // earlier in raster order: s >= s_q
      const int after = max(max((int)m[1], (int)m[kSP - 1]), max((int)m[kSP], (int)m[kSP + 1]));        // later: s > s_q
      take = s >= before && s > after;
    }
    if (MASK && take) take = ((tmask[r] >> q) & 1ull) == 0;
    const unsigned long long act = __ballot(take);
    if (act) {
      const int leader = __ffsll((long long)act) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(&s_cnt, __popcll(act));
      base = __shfl(base, leader, kWave);
      const int pos = base + __popcll(act & ((1ull << lane) - 1ull));
      if (take && pos < kTileCand)   // the bound never binds: no two candidates are neighbours
        keys[pos] = ((unsigned long long)__float_as_uint((float)s) << 32) | (unsigned)(y * w + x);
    }
  }
  __syncthreads();
  const int n = min(s_cnt, kTileCand);
  if (n == 0) return;
  if (tid == 0) s_base = atomicAdd(&cand_count[blockIdx.y], n);
  __syncthreads();
  const int base = s_base;
  unsigned long long* out = cand + (size_t)blockIdx.y * c.cap;
  for (int k = tid; k < n; k += kThreads)
    if (base + k < c.cap) out[base + k] = keys[k];   // never binds either
}

// Step 5.  A thread owns keep rows 4 tid .. 4 tid + 3 (max_kp <= 4096): liveness, an exclusive scan over the workgroup, then every entry
// of every output of the image.
__global__ __launch_bounds__(1024) void k_fast_merge(const float* __restrict__ keep, const int* __restrict__ keep_n, int unit_stride,
                                                     int max_kp, const float* __restrict__ new_kp, const int* __restrict__ n_new, int max_new,
                                                     int target, float* __restrict__ kp_out, int* __restrict__ n_out,
                                                     int* __restrict__ carry0) {
  __shared__ int wave_tot[1024 / kWave];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int n_keep = keep ? min(max(keep_n[(size_t)img * unit_stride], 0), max_kp) : 0;
  const float* rows = keep ? keep + (size_t)img * unit_stride * max_kp * 3 : nullptr;
  float v[4][3];
  bool live[4];
  int mine = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = 4 * tid + j;
    live[j] = false;
    if (i < n_keep) {
      v[j][0] = rows[3 * i]; v[j][1] = rows[3 * i + 1]; v[j][2] = rows[3 * i + 2];
      live[j] = fast_coord_ok(v[j][0]) && fast_coord_ok(v[j][1]);
    }
    mine += live[j];
  }
  int incl = mine;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int up = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += up;
  }
  if (lane == kWave - 1) wave_tot[wave] = incl;
  __syncthreads();
  int before = incl - mine, L = 0;
  for (int q = 0; q < 1024 / kWave; ++q) {
    const int t = wave_tot[q];
    if (q < wave) before += t;
    L += t;
  }
  const int K = min(max(n_new[img], 0), max_new);
  int A = min(K, max_kp - L);
  if (target > 0) A = min(A, max(0, target - L));
  float* out = kp_out + (size_t)img * max_kp * 3;
  int pos = before;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = 4 * tid + j;
    if (i >= max_kp) break;
    if (live[j]) { out[3 * pos] = v[j][0]; out[3 * pos + 1] = v[j][1]; out[3 * pos + 2] = v[j][2]; }
    if (carry0) carry0[(size_t)img * max_kp + i] = live[j] ? pos : -1;
    pos += live[j];
  }
  const float* src = new_kp + (size_t)img * max_new * 3;
  for (int i = L + tid; i < max_kp; i += 1024) {
    const bool fresh = i < L + A;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * i + k] = fresh ? src[3 * (i - L) + k] : 0.f;
  }
  if (tid == 0) n_out[img] = L + A;
}

static bool dword_rows(const void* p, long long image_stride, long long stride) {
  return (reinterpret_cast<uintptr_t>(p) | (uintptr_t)image_stride | (uintptr_t)stride) % 4 == 0;
}

void launch_fast_score(const uint8_t* imgs, long long image_stride, long long stride, int h, int w, uint8_t* score,
                       long long score_image_stride, long long score_stride, int images, hipStream_t s) {
  const int tiles_x = (w + kTW - 1) / kTW, tiles_y = (h + kTH - 1) / kTH;
  const dim3 grid(tiles_x * tiles_y, images);
  if (dword_rows(imgs, image_stride, stride))
    hipLaunchKernelGGL(k_fast_score<true>, grid, dim3(kThreads), 0, s, imgs, image_stride, stride, h, w, tiles_x, score, score_image_stride, score_stride);
  else
    hipLaunchKernelGGL(k_fast_score<false>, grid, dim3(kThreads), 0, s, imgs, image_stride, stride, h, w, tiles_x, score, score_image_stride, score_stride);
}

void launch_fast_detect(const uint8_t* imgs, long long image_stride, long long stride, const FastK& c, const float* keep, const int* keep_n,
                        unsigned long long* cand, int* cand_count, int images, hipStream_t s) {
  const dim3 grid(c.tiles_x * c.tiles_y, images);
  const bool a4 = dword_rows(imgs, image_stride, stride), masked = keep && c.min_distance > 0;
#define SSHIP_FAST_DETECT(A4, M) \
  hipLaunchKernelGGL((k_fast_detect<A4, M>), grid, dim3(kThreads), 0, s, imgs, image_stride, stride, c, keep, keep_n, cand, cand_count)
  if (a4 && masked) SSHIP_FAST_DETECT(true, true);
  else if (a4) SSHIP_FAST_DETECT(true, false);
  else if (masked) SSHIP_FAST_DETECT(false, true);
  else SSHIP_FAST_DETECT(false, false);
#undef SSHIP_FAST_DETECT
}

void launch_fast_merge(const float* keep, const int* keep_n, int unit_stride, int max_kp, const float* new_kp, const int* n_new, int max_new,
                       int target, float* kp_out, int* n_out, int* carry0, int images, hipStream_t s) {
  hipLaunchKernelGGL(k_fast_merge, dim3(images), dim3(1024), 0, s, keep, keep_n, unit_stride, max_kp, new_kp, n_new, max_new, target, kp_out, n_out,
                     carry0);
}

}  // namespace sship
