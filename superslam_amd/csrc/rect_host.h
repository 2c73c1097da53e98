// Pure host half of the rectifier (include/sship.h "Rectification"): the map builder, the fixed-point table and the per-tile source
// boxes.  Plain C++17, no HIP: api.hip includes it, and tests/cpp/test_rect_host.cc builds it alone (also under the host sanitizers).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace sship {

constexpr int kRectMaxSize = 4096;    // source and destination sizes: [1, 4096] on each axis
constexpr int kRectTileW = 64;        // destination tile of one workgroup: 64 x 16 pixels, 4 consecutive pixels per lane
constexpr int kRectTileH = 16;
constexpr int kRectLdsBytes = 16384;  // a tile whose staged source box (rows x pitch) exceeds this takes the direct path
constexpr uint16_t kRectFracMask = 1023;

// one destination pixel of the device table: the top-left tap (int16 each; a pixel with no tap inside the source is (-2, -2)),
// the weights ax | ay << 5, and bits 10..13 = the taps that are inside the source AND have a non-zero weight
// (bit 0: (ix, iy), 1: (ix + 1, iy), 2: (ix, iy + 1), 3: (ix + 1, iy + 1)).  The kernel reads exactly the taps of that mask.
struct RectEntry { int16_t ix, iy; uint32_t frac_mask; };
static_assert(sizeof(RectEntry) == 8, "the kernel loads an entry as one uint2");
// the source box of one tile: every masked tap of its pixels lies in [x0, x0 + bw) x [y0, y0 + bh); bh == 0: no tap at all
struct RectTile { int x0, y0, bw, bh, direct, pad0, pad1, pad2; };

inline int rect_box_pitch(int bw) { return (bw + 6) & ~3; }   // LDS bytes per staged row: bw + the row's misalignment (<= 3), in whole dwords

// Steps 1-5 of the rule, in this operation order (tests/_rect_ref.py restates it).  Returns 0, or 1 when Pnew * R is singular / not finite.
inline int rect_build_maps(const double* K, const double* D, int n_dist, const double* R, const double* Pnew, int dst_w, int dst_h,
                           float* map_x, float* map_y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  static const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const double* Rm = R ? R : I3;
  double A[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[3 * i + j] = (Pnew[3 * i] * Rm[j] + Pnew[3 * i + 1] * Rm[3 + j]) + Pnew[3 * i + 2] * Rm[6 + j];
  // inverse by cofactors: iR = adj(A) / det
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double det = (A[0] * c00 + A[1] * c01) + A[2] * c02;
  if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return 1;
  const double iR[9] = {c00 / det, (A[2] * A[7] - A[1] * A[8]) / det, (A[1] * A[5] - A[2] * A[4]) / det,
                        c01 / det, (A[0] * A[8] - A[2] * A[6]) / det, (A[2] * A[3] - A[0] * A[5]) / det,
                        c02 / det, (A[1] * A[6] - A[0] * A[7]) / det, (A[0] * A[4] - A[1] * A[3]) / det};
  for (double v : iR)
    if (!std::isfinite(v)) return 1;
  double d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n_dist; ++i) d[i] = D[i];
  const double k1 = d[0], k2 = d[1], p1 = d[2], p2 = d[3], k3 = d[4], k4 = d[5], k5 = d[6], k6 = d[7];
  const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
  for (int v = 0; v < dst_h; ++v)
    for (int u = 0; u < dst_w; ++u) {
      const double X = (iR[0] * u + iR[1] * v) + iR[2], Y = (iR[3] * u + iR[4] * v) + iR[5], W = (iR[6] * u + iR[7] * v) + iR[8];
      const double x = X / W, y = Y / W;
      const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = (2.0 * x) * y;
      const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
      const double xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2);
      const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2;
      map_x[(size_t)v * dst_w + u] = (float)(fx * xd + cx);
      map_y[(size_t)v * dst_w + u] = (float)(fy * yd + cy);
    }
  return 0;
}

// One map value to fixed point: s = rint(m * 32) (fp32 product, exact; ties to even under the default rounding mode).
// false: the entry is degenerate (not finite, or |m * 32| > 2^20) and its pixel is 0.
inline bool rect_fixed(float m, int32_t* s) {
  const float p = m * 32.0f;
  if (!std::isfinite(p) || std::fabs(p) > 1048576.0f) { *s = 0; return false; }
  *s = (int32_t)std::nearbyintf(p);
  return true;
}
// the table as the rule states it: ix = sx >> 5, iy = sy >> 5, frac = ax | ay << 5; degenerate entries: ix = iy = 0, frac = 0xFFFF
inline void rect_fixed_table(const float* map_x, const float* map_y, size_t count, int32_t* ix, int32_t* iy, uint16_t* frac) {
  for (size_t i = 0; i < count; ++i) {
    int32_t sx, sy;
    const bool okx = rect_fixed(map_x[i], &sx), oky = rect_fixed(map_y[i], &sy);
    if (okx && oky) { ix[i] = sx >> 5; iy[i] = sy >> 5; frac[i] = (uint16_t)((sx & 31) | ((sy & 31) << 5)); }
    else { ix[i] = 0; iy[i] = 0; frac[i] = 0xFFFF; }
  }
}

// The device table and the tile boxes of one camera.  tiles: [tiles_y][tiles_x], row-major.
inline void rect_device_table(const float* map_x, const float* map_y, int src_w, int src_h, int dst_w, int dst_h,
                              std::vector<RectEntry>& table, std::vector<RectTile>& tiles, int* n_staged, int* n_direct) {
  const int tx_n = (dst_w + kRectTileW - 1) / kRectTileW, ty_n = (dst_h + kRectTileH - 1) / kRectTileH;
  table.assign((size_t)dst_w * dst_h, RectEntry{-2, -2, 0});
  tiles.assign((size_t)tx_n * ty_n, RectTile{0, 0, 0, 0, 0, 0, 0, 0});
  *n_staged = *n_direct = 0;
  for (int ty = 0; ty < ty_n; ++ty)
    for (int tx = 0; tx < tx_n; ++tx) {
      int xmin = src_w, xmax = -1, ymin = src_h, ymax = -1;
      for (int v = ty * kRectTileH; v < std::min(dst_h, (ty + 1) * kRectTileH); ++v)
        for (int u = tx * kRectTileW; u < std::min(dst_w, (tx + 1) * kRectTileW); ++u) {
          const size_t i = (size_t)v * dst_w + u;
          int32_t sx, sy;
          if (!rect_fixed(map_x[i], &sx) || !rect_fixed(map_y[i], &sy)) continue;   // degenerate: stays (-2, -2, no tap)
          const int ix = sx >> 5, iy = sy >> 5, ax = sx & 31, ay = sy & 31;
          uint32_t mask = 0;
          for (int t = 0; t < 4; ++t) {
            const int x = ix + (t & 1), y = iy + (t >> 1);
            const int w = ((t & 1) ? ax : 32 - ax) * ((t >> 1) ? ay : 32 - ay);
            if (w != 0 && x >= 0 && x < src_w && y >= 0 && y < src_h) {
              mask |= 1u << t;
              xmin = std::min(xmin, x); xmax = std::max(xmax, x); ymin = std::min(ymin, y); ymax = std::max(ymax, y);
            }
          }
          if (mask) table[i] = RectEntry{(int16_t)ix, (int16_t)iy, (uint32_t)(ax | (ay << 5)) | (mask << 10)};   // -1 <= ix < src_w <= 4096
        }
      RectTile& t = tiles[(size_t)ty * tx_n + tx];
      if (xmax >= 0) {
        t.x0 = xmin; t.y0 = ymin; t.bw = xmax - xmin + 1; t.bh = ymax - ymin + 1;
        t.direct = (long long)t.bh * rect_box_pitch(t.bw) > kRectLdsBytes ? 1 : 0;
        ++*(t.direct ? n_direct : n_staged);
      } else {
        ++*n_staged;   // nothing to read: the staged loop stages nothing and writes zeros
      }
    }
}

}  // namespace sship
