// Contrast-limited adaptive histogram equalisation (include/sship.h "CLAHE").
//   k_clahe_lut<ALIGNED>        one 256-thread workgroup builds the 256-byte table of one tile of one image: grid (tiles, images).
//   k_clahe_apply<SRC4, DST4>   one 256-thread workgroup owns a block of 256 x 32 destination pixels (fewer rows for tiny tiles) of one
//                               image: grid (blocks, images).
//
// k_clahe_lut counts the tile's pixels of the extended image (every index through reflect-101, so no load leaves the image) into four
// sub-histograms in LDS, one per wave, with LDS atomics: on a low-entropy tile the 64 lanes of a wave already queue on a few counters, four
// waves on one copy would queue four times as long.  A thread walks (row, dword) units of the tile: with ALIGNED (pointer, image stride
// and row stride multiples of 4, picked on the host per launch) a dword that lies whole inside the tile and the image is one load, every
// other unit and every unit without ALIGNED goes byte by byte; four units' loads are issued before their counts.  Four equal bytes are one
// atomic of 4.  Then thread v owns bin v: the four
// copies are added, the excess over the limit is summed over the workgroup (integers: any order), the bin is clipped and given its share,
// a 256-wide inclusive scan (shuffles inside a wave, three wave totals through LDS) gives s_v, and the table byte is one fp32 product
// rounded to nearest even.  Counts are 32-bit: a tile may hold 2^24 equal pixels.  4 128 B of static LDS, no scratch.
//
// k_clahe_apply works on cells: the pixels between two tile-centre lines on each axis share the rule's four tables, and a cell holds them
// interleaved - dword v of a cell is (lut11[v], lut12[v], lut21[v], lut22[v]) - so a pixel is ONE LDS gather (a dword) and four byte-to-
// float conversions in place of four byte gathers.  A block stages the cells its pixels touch (found with the rule's own fp32
// expressions at the block's first and last pixel) in dynamic LDS: a thread reads four values of the four tables as four dwords and
// writes them byte-transposed as one 16-byte store.  The host sizes the LDS from the block and tile sizes and picks the block's height
// (32, 16, ... 1 rows) so that at most 64 cells (64 KiB) are staged: 6 cells (6 KiB) and 32 rows at 1376 x 376 with 8 x 8 tiles; only
// tiles of a few pixels lower the block.  A thread owns four neighbouring pixels of a row and every fourth row of the block, and loads
// all its rows before it computes (a dword per lane is a narrow load: eight of them in flight); the x half
// of the interpolation (the cell column and two weights per pixel) is formed once and kept in registers.  Each pixel is seven fp32
// operations, each rounded once (the file is compiled with -ffp-contract=off).  Source and destination are read and written as whole
// dwords where pointer and strides allow it (SRC4 / DST4, picked on the host per launch), byte by byte otherwise and in a row's last
// partial group: nothing outside w bytes of a row is touched.  A thread reads only the four pixels it writes, so the call may run in
// place.  The scale, the limit and the two reciprocals come from the host by value: no device division enters the rule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace sship {

namespace {
constexpr int kThreads = 256, kWaves = kThreads / kWave, kBatch = 4;

// reflect-101 for an index of the extended image: the host refused sizes where one reflection does not land inside
__device__ __forceinline__ int reflect_ext(int i, int n) { return i < n ? i : 2 * (n - 1) - i; }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}
}  // namespace

template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_clahe_lut(const uint8_t* __restrict__ src, long long image_stride, long long stride, int h, int w,
                                                   ClaheK c, uint8_t* __restrict__ luts) {
  __shared__ uint32_t hist[kWaves * 256];
  __shared__ int part[2 * kWaves];
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  const int tj = blockIdx.x / c.tiles_x, ti = blockIdx.x - tj * c.tiles_x;
  for (int k = tid; k < kWaves * 256; k += kThreads) hist[k] = 0;
  __syncthreads();
  uint32_t* mine = hist + wave * 256;
  const uint8_t* s = src + (size_t)blockIdx.y * image_stride;
  const int c0 = ti * c.tw, c1 = c0 + c.tw, r0 = tj * c.th;
  const int d0 = c0 >> 2, nd = ((c1 - 1) >> 2) - d0 + 1;   // the dwords (counted from the row's start) that the tile's columns touch
  const int units = c.th * nd;                             // <= 16 400 x 4 101
  // four units per pass: the whole dwords are loaded first and counted afterwards, so that a thread has four loads in flight
  for (int k0 = tid; k0 < units; k0 += kBatch * kThreads) {
    uint32_t val[kBatch];
    bool whole[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int k = k0 + j * kThreads;
      whole[j] = false;
      if (k >= units) continue;
      const int r = k / nd, d = k - r * nd;
      const uint8_t* row = s + (size_t)reflect_ext(r0 + r, h) * stride;
      const int x = 4 * (d0 + d);
      if (x >= c0 && x + 3 < c1 && x + 3 < w) {
        whole[j] = true;
        if (ALIGNED) val[j] = *reinterpret_cast<const uint32_t*>(row + x);
        else val[j] = (uint32_t)row[x] | (uint32_t)row[x + 1] << 8 | (uint32_t)row[x + 2] << 16 | (uint32_t)row[x + 3] << 24;
      } else {                                             // a dword across the tile's or the image's edge: byte by byte, at once
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int xe = x + b;
          if (xe >= c0 && xe < c1) atomicAdd(&mine[row[reflect_ext(xe, w)]], 1u);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      if (!whole[j]) continue;
      const uint32_t v = val[j];
      if (v == (v & 255u) * 0x01010101u) {
        atomicAdd(&mine[v & 255u], 4u);
      } else {
        atomicAdd(&mine[v & 255u], 1u); atomicAdd(&mine[(v >> 8) & 255u], 1u);
        atomicAdd(&mine[(v >> 16) & 255u], 1u); atomicAdd(&mine[v >> 24], 1u);
      }
    }
  }
  __syncthreads();
  // thread v owns bin v from here on
  int cnt = (int)(hist[tid] + hist[256 + tid] + hist[512 + tid] + hist[768 + tid]);
  if (c.limit > 0) {
    const int over = wave_sum(cnt > c.limit ? cnt - c.limit : 0);
    if (lane == 0) part[wave] = over;
    __syncthreads();
    const int clipped = part[0] + part[1] + part[2] + part[3];
    const int batch = clipped >> 8, residual = clipped & 255;
    cnt = (cnt < c.limit ? cnt : c.limit) + batch;
    if (residual > 0) {
      const int step = 256 / residual;                     // >= 1: residual <= 255
      const int q = tid / step;
      if (q * step == tid && q < residual) cnt += 1;
    }
  }
  // inclusive scan over the 256 bins
  int sum = cnt;
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    const int o = __shfl_up(sum, m, kWave);
    if (lane >= m) sum += o;
  }
  if (lane == kWave - 1) part[kWaves + wave] = sum;
  __syncthreads();
  for (int q = 0; q < wave; ++q) sum += part[kWaves + q];
  const float f = fminf(fmaxf(rintf((float)sum * c.scale), 0.f), 255.f);
  luts[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid] = (uint8_t)(int)f;
}

namespace {
constexpr int kMaxCells = 64;                              // 64 cells x 256 dwords = 64 KiB of dynamic LDS at the most

// A cell is what the pixels between two tile-centre lines on each axis share: the four tables of the rule.  Along an axis it is named by
// t1 + 1 in 0 .. tiles (t1 = -1 left of the first centre line), and holds the tables max(t1, 0) and min(t1 + 1, tiles - 1).
struct AxisW { int cell; float a, a1; };
__device__ __forceinline__ int axis_t1(float f, int tiles) { return min(max((int)floorf(f), -1), tiles - 1); }   // the clamp never binds
// the rule's weights of pixel coordinate i and its cell, counted from the first cell the block staged (n of them)
__device__ __forceinline__ AxisW axis_weights(int i, float inv, int tiles, int lo, int n) {
  const float f = (float)i * inv - 0.5f;
  AxisW r;
  r.a = f - floorf(f);
  r.a1 = 1.0f - r.a;
  r.cell = min(max(axis_t1(f, tiles) + 1 - lo, 0), n - 1);   // the clamp never binds: it keeps the index inside the staged block whatever happens
  return r;
}
__device__ __forceinline__ int axis_cell(int i, float inv, int tiles) { return axis_t1((float)i * inv - 0.5f, tiles) + 1; }
// byte k of a, b, c, d -> one dword
__device__ __forceinline__ uint32_t pack_bytes(uint32_t a, uint32_t b, uint32_t c, uint32_t d, int k) {
  return ((a >> (8 * k)) & 255u) | ((b >> (8 * k)) & 255u) << 8 | ((c >> (8 * k)) & 255u) << 16 | ((d >> (8 * k)) & 255u) << 24;
}
}  // namespace

template <bool SRC4, bool DST4>
__global__ __launch_bounds__(256) void k_clahe_apply(const uint8_t* src, long long src_image_stride, long long src_stride, uint8_t* dst,
                                                     long long dst_image_stride, long long dst_stride, int h, int w, ClaheK c,
                                                     const uint8_t* __restrict__ luts, int blocks_x, int block_h, int cap_x, int cap_y) {
  extern __shared__ uint4 cells16[];
  const uint32_t* cells = reinterpret_cast<const uint32_t*>(cells16);
  const int tid = threadIdx.x;
  const int by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
  const int X0 = bx * kClaheBlockW, Y0 = by * block_h;
  const int X1 = min(X0 + kClaheBlockW, w) - 1, Y1 = min(Y0 + block_h, h) - 1;
  const int cx_lo = axis_cell(X0, c.inv_tw, c.tiles_x), cy_lo = axis_cell(Y0, c.inv_th, c.tiles_y);
  const int nx = min(axis_cell(X1, c.inv_tw, c.tiles_x) - cx_lo + 1, cap_x), ny = min(axis_cell(Y1, c.inv_th, c.tiles_y) - cy_lo + 1, cap_y);
  const int x = X0 + 4 * (tid % 64), px = min(4, w - x);
  const uint8_t* s = src + (size_t)blockIdx.y * src_image_stride;
  uint8_t* o = dst + (size_t)blockIdx.y * dst_image_stride;
  // every row's load first (8 in flight per thread at the full block height), ahead of the staging; the arithmetic after it
  constexpr int kRows = kClaheBlockH / (kThreads / 64);
  const int y0 = Y0 + tid / 64;
  uint32_t val[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int y = y0 + r * (kThreads / 64);
    val[r] = 0;
    if (y > Y1 || x >= w) continue;
    const uint8_t* sr = s + (size_t)y * src_stride + x;
    if (SRC4 && px == 4) val[r] = *reinterpret_cast<const uint32_t*>(sr);
    else
      for (int b = 0; b < px; ++b) val[r] |= (uint32_t)sr[b] << (8 * b);
  }
  // stage the cells: a thread reads values 4 q .. 4 q + 3 of a cell's four tables as four dwords and writes them byte-transposed
  const uint32_t* g = reinterpret_cast<const uint32_t*>(luts + (size_t)blockIdx.y * c.tiles_x * c.tiles_y * 256);
  for (int k = tid; k < nx * ny * 64; k += kThreads) {
    const int cell = k >> 6, q = k & 63, cy = cell / nx, cx = cell - cy * nx;
    const int ty1 = max(cy_lo + cy - 1, 0), ty2 = min(cy_lo + cy, c.tiles_y - 1), tx1 = max(cx_lo + cx - 1, 0), tx2 = min(cx_lo + cx, c.tiles_x - 1);
    const uint32_t l11 = g[(ty1 * c.tiles_x + tx1) * 64 + q], l12 = g[(ty1 * c.tiles_x + tx2) * 64 + q];
    const uint32_t l21 = g[(ty2 * c.tiles_x + tx1) * 64 + q], l22 = g[(ty2 * c.tiles_x + tx2) * 64 + q];
    cells16[k] = make_uint4(pack_bytes(l11, l12, l21, l22, 0), pack_bytes(l11, l12, l21, l22, 1), pack_bytes(l11, l12, l21, l22, 2),
                            pack_bytes(l11, l12, l21, l22, 3));
  }
  __syncthreads();
  if (x >= w) return;
  AxisW ax[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) ax[b] = axis_weights(min(x + b, w - 1), c.inv_tw, c.tiles_x, cx_lo, nx);
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int y = y0 + r * (kThreads / 64);
    if (y > Y1) continue;
    uint8_t* dr = o + (size_t)y * dst_stride + x;
    const uint32_t v = val[r];
    const AxisW ay = axis_weights(y, c.inv_th, c.tiles_y, cy_lo, ny);
    const uint32_t* row = cells + ay.cell * nx * 256;
    uint32_t out = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t l = row[ax[b].cell * 256 + ((v >> (8 * b)) & 255u)];
      const float l11 = (float)(l & 255u), l12 = (float)((l >> 8) & 255u), l21 = (float)((l >> 16) & 255u), l22 = (float)(l >> 24);
      const float top = l11 * ax[b].a1 + l12 * ax[b].a, bot = l21 * ax[b].a1 + l22 * ax[b].a;
      const float res = top * ay.a1 + bot * ay.a;
      out |= (uint32_t)(int)fminf(fmaxf(rintf(res), 0.f), 255.f) << (8 * b);
    }
    if (DST4 && px == 4) *reinterpret_cast<uint32_t*>(dr) = out;
    else
      for (int b = 0; b < px; ++b) dr[b] = (uint8_t)(out >> (8 * b));
  }
}

// dword loads and stores need every row of every image on a multiple of 4 bytes
static bool dword_rows(const void* p, long long image_stride, long long stride) {
  return (reinterpret_cast<uintptr_t>(p) | (uintptr_t)image_stride | (uintptr_t)stride) % 4 == 0;
}

// The pixel kernel's block is 256 pixels wide and block_h = 32, 16, ... 1 rows high: the highest whose cells fit kMaxCells.  Pixels i and
// i + B - 1 lie (B - 1) / t tile widths apart, so their t1 differ by at most (B - 1) / t + 1: (B - 1) / t + 2 cells, and never more than
// tiles + 1.  Two rows touch at most 3 cells in y and 256 pixels at most 17 in x: block_h = 2 always fits.
static void clahe_apply_shape(const ClaheK& c, int* block_h, int* cap_x, int* cap_y) {
  *cap_x = std::min(c.tiles_x + 1, (kClaheBlockW - 1) / c.tw + 2);
  for (*block_h = kClaheBlockH;; *block_h >>= 1) {
    *cap_y = std::min(c.tiles_y + 1, (*block_h - 1) / c.th + 2);
    if (*cap_x * *cap_y <= kMaxCells || *block_h == 1) return;
  }
}
void launch_clahe_lut(const uint8_t* src, long long src_image_stride, long long src_stride, int h, int w, const ClaheK& c, uint8_t* luts,
                      int images, hipStream_t s) {
  const dim3 grid(c.tiles_x * c.tiles_y, images);
  if (dword_rows(src, src_image_stride, src_stride))
    hipLaunchKernelGGL(k_clahe_lut<true>, grid, dim3(kThreads), 0, s, src, src_image_stride, src_stride, h, w, c, luts);
  else
    hipLaunchKernelGGL(k_clahe_lut<false>, grid, dim3(kThreads), 0, s, src, src_image_stride, src_stride, h, w, c, luts);
}

void launch_clahe_apply(const uint8_t* src, long long src_image_stride, long long src_stride, uint8_t* dst, long long dst_image_stride,
                        long long dst_stride, int h, int w, const ClaheK& c, const uint8_t* luts, int images, hipStream_t s) {
  const bool s4 = dword_rows(src, src_image_stride, src_stride), d4 = dword_rows(dst, dst_image_stride, dst_stride);
  int block_h, cap_x, cap_y;
  clahe_apply_shape(c, &block_h, &cap_x, &cap_y);
  const int blocks_x = (w + kClaheBlockW - 1) / kClaheBlockW, blocks_y = (h + block_h - 1) / block_h;
  const dim3 grid(blocks_x * blocks_y, images);
  const size_t lds = (size_t)cap_x * cap_y * 1024;
#define SSHIP_CLAHE_APPLY(S4, D4)                                                                                                              \
  hipLaunchKernelGGL((k_clahe_apply<S4, D4>), grid, dim3(kThreads), lds, s, src, src_image_stride, src_stride, dst, dst_image_stride, dst_stride, \
                     h, w, c, luts, blocks_x, block_h, cap_x, cap_y)
  if (s4 && d4) SSHIP_CLAHE_APPLY(true, true);
  else if (s4) SSHIP_CLAHE_APPLY(true, false);
  else if (d4) SSHIP_CLAHE_APPLY(false, true);
  else SSHIP_CLAHE_APPLY(false, false);
#undef SSHIP_CLAHE_APPLY
}

}  // namespace sship
