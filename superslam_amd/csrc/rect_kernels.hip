// Rectification remap and RGB-D depth association (include/sship.h "Rectification" / "RGB-D association").
//   k_rect_remap      one workgroup = one 64 x 16 destination tile of one camera and a slice of that camera's images.  The tile's table
//                     entries stay in registers across the image loop; per image the tile's source box is staged into LDS with dword
//                     loads (staged path) or the taps are read from global memory (direct path: boxes over the LDS budget).
//   k_rgbd_associate  one thread per keypoint slot, fp64.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace sship {

// a staged source row r of the box starts at byte address A_r = img + (y0 + r) * stride + x0; LDS row r holds the aligned dwords from
// A_r & ~3 on, so box pixel (r, c) is at LDS byte r * pitch + (A_r & 3) + c, pitch = rect_box_pitch(bw) >= bw + 3.
__global__ __launch_bounds__(256) void k_rect_remap(const uint8_t* __restrict__ src, long long img_bytes, int src_stride,
                                                    uint8_t* __restrict__ dst, int dst_w, int dst_h, const uint2* __restrict__ table,
                                                    const RectTile* __restrict__ tiles, int tiles_x, int tiles_y, int cameras, int cam0,
                                                    int images, int force_direct) {
  __shared__ uint32_t lds32[kRectLdsBytes / 4];
  const uint8_t* lds8 = reinterpret_cast<const uint8_t*>(lds32);
  const int tid = threadIdx.x;
  const int per_cam = tiles_x * tiles_y;
  const int cam = blockIdx.x / per_cam, tile = blockIdx.x - cam * per_cam;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int first = (cam - cam0 % cameras + cameras) % cameras;   // first image of the batch that uses this camera
  if (first >= images) return;
  const int n_img = (images - first + cameras - 1) / cameras;
  const RectTile t = tiles[blockIdx.x];
  const bool direct = force_direct || t.direct;
  const int pitch = (t.bw + 6) & ~3, pdw = pitch >> 2;

  const int x = tx * kRectTileW + (tid & 15) * 4, y = ty * kRectTileH + (tid >> 4);
  // this lane's four pixels: tap mask / weights, LDS offset of the top-left tap, and the tap itself for the direct path
  uint32_t fm[4];
  int l0[4], tix[4], tiy[4];
  uint32_t q[4];   // (A_r & 3) without the image base, for the tap's two rows: bits 0..1 and 2..3
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    fm[j] = 0; l0[j] = 0; tix[j] = 0; tiy[j] = 0; q[j] = 0;
    if (y < dst_h && x + j < dst_w) {
      const uint2 e = table[(size_t)cam * dst_w * dst_h + (size_t)y * dst_w + x + j];
      tix[j] = (int)(int16_t)(e.x & 0xffffu); tiy[j] = (int)(int16_t)(e.x >> 16);
      fm[j] = e.y;
      l0[j] = (tiy[j] - t.y0) * pitch + (tix[j] - t.x0);
      const uint32_t r0 = (uint32_t)tiy[j] * (uint32_t)src_stride + (uint32_t)t.x0;
      q[j] = (r0 & 3u) | (((r0 + (uint32_t)src_stride) & 3u) << 2);
    }
  }
  const uint8_t* lo = src;
  const uint8_t* hi = src + (long long)images * img_bytes;   // dword loads stay inside [lo, hi): the extent the caller stated

  for (int k = blockIdx.y; k < n_img; k += gridDim.y) {
    const int img = first + k * cameras;
    const uint8_t* sb = src + (long long)img * img_bytes;
    if (!direct) {
      __syncthreads();   // the previous image's gathers are done
      const int total = t.bh * pdw;
      for (int e = tid; e < total; e += 256) {
        const int r = e / pdw, d = e - r * pdw;
        const uint8_t* a = sb + (long long)(t.y0 + r) * src_stride + t.x0;
        const int sh = (int)(reinterpret_cast<uintptr_t>(a) & 3);
        if (d * 4 < sh + t.bw) {
          const uint8_t* p = a - sh + d * 4;
          uint32_t v;
          if (p >= lo && p + 4 <= hi) {
            v = *reinterpret_cast<const uint32_t*>(p);
          } else {   // the dword straddles the stated extent: its bytes one by one
            v = 0;
            for (int b = 0; b < 4; ++b)
              if (p + b >= lo && p + b < hi) v |= (uint32_t)p[b] << (8 * b);
          }
          lds32[e] = v;
        }
      }
      __syncthreads();
    }
    const uint32_t base = (uint32_t)(reinterpret_cast<uintptr_t>(sb) & 3);
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t m = fm[j] >> 10;
      uint32_t p00 = 0, p01 = 0, p10 = 0, p11 = 0;
      if (direct) {
        const uint8_t* p = sb + (long long)tiy[j] * src_stride + tix[j];
        if (m & 1) p00 = p[0];
        if (m & 2) p01 = p[1];
        if (m & 4) p10 = p[src_stride];
        if (m & 8) p11 = p[src_stride + 1];
      } else {
        const int a0 = l0[j] + (int)((base + q[j]) & 3u), a1 = l0[j] + pitch + (int)((base + (q[j] >> 2)) & 3u);
        if (m & 1) p00 = lds8[a0];
        if (m & 2) p01 = lds8[a0 + 1];
        if (m & 4) p10 = lds8[a1];
        if (m & 8) p11 = lds8[a1 + 1];
      }
      const uint32_t ax = fm[j] & 31u, ay = (fm[j] >> 5) & 31u;
      const uint32_t acc = (32u - ay) * ((32u - ax) * p00 + ax * p01) + ay * ((32u - ax) * p10 + ax * p11);
      out |= ((acc + 512u) >> 10) << (8 * j);
    }
    if (y < dst_h && x < dst_w) {
      uint8_t* o = dst + ((size_t)img * dst_h + y) * dst_w + x;
      if (x + 3 < dst_w && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(o) = out;
      } else {
        for (int j = 0; j < 4; ++j)
          if (x + j < dst_w) o[j] = (uint8_t)(out >> (8 * j));
      }
    }
  }
}

void launch_rect_remap(const uint8_t* src, int src_h, int src_stride, uint8_t* dst, int dst_w, int dst_h, const void* table,
                       const RectTile* tiles, int cameras, int cam0, int images, int force_direct, hipStream_t s) {
  const int tiles_x = (dst_w + kRectTileW - 1) / kRectTileW, tiles_y = (dst_h + kRectTileH - 1) / kRectTileH;
  const int total = tiles_x * tiles_y * cameras;
  const int per_cam = (images + cameras - 1) / cameras;
  // enough workgroups for 256 CUs x 8: the image loop is split into slices only while the tiles alone are too few
  int slices = (2048 + total - 1) / total;
  slices = slices < 1 ? 1 : (slices > per_cam ? per_cam : slices);
  hipLaunchKernelGGL(k_rect_remap, dim3(total, slices), dim3(256), 0, s, src, (long long)src_h * src_stride, src_stride, dst, dst_w, dst_h,
                     static_cast<const uint2*>(table), tiles, tiles_x, tiles_y, cameras, cam0, images, force_direct);
}

template <class T>
__device__ inline double depth_at(const void* depth, long long off_bytes) {
  return (double)*reinterpret_cast<const T*>(static_cast<const uint8_t*>(depth) + off_bytes);
}

__global__ __launch_bounds__(256) void k_rgbd_associate(const float* __restrict__ kp, const int* __restrict__ lens, int R,
                                                        const void* __restrict__ depth, int depth_f32, int h, int w, long long depth_stride,
                                                        RgbdK c, float* __restrict__ kp_undist, float* __restrict__ stereo,
                                                        uint8_t* __restrict__ has_depth) {
  const int frame = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  const int n = min(max(lens[frame], 0), R);
  const size_t row = (size_t)frame * R + i;
  float u = 0.f, v = 0.f, score = 0.f, uR = __builtin_nanf("");
  bool hd = false;
  if (i < n) {
    const float ur = kp[row * 3], vr = kp[row * 3 + 1];
    score = kp[row * 3 + 2];
    u = ur; v = vr;
    if (c.has_dist) {
      const double k1 = c.d[0], k2 = c.d[1], p1 = c.d[2], p2 = c.d[3], k3 = c.d[4], k4 = c.d[5], k5 = c.d[6], k6 = c.d[7];
      const double x0 = ((double)ur - c.cx) / c.fx, y0 = ((double)vr - c.cy) / c.fy;
      double x = x0, y = y0;
      for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double ic = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        if (ic < 0.0) { x = x0; y = y0; break; }
        const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x), dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - dx) * ic; y = (y0 - dy) * ic;
      }
      u = (float)(c.fx * x + c.cx); v = (float)(c.fy * y + c.cy);
    }
    const float ru = roundf(ur), rv = roundf(vr);   // lround: half away from zero
    double Z = 0.0;
    if (ru >= 0.f && ru < (float)w && rv >= 0.f && rv < (float)h) {   // NaN coordinates: outside
      const long long off = (long long)(int)rv * depth_stride;
      const double dv = depth_f32 ? depth_at<float>(depth, (long long)frame * h * depth_stride + off + (long long)(int)ru * 4)
                                  : depth_at<uint16_t>(depth, (long long)frame * h * depth_stride + off + (long long)(int)ru * 2);
      Z = dv / c.depth_factor;
    }
    hd = Z > 0.0 && Z < c.max_depth;   // the positive form: NaN gives no depth
    if (hd) uR = (float)((double)u - c.bf / Z);
  }
  stereo[row * 3] = u; stereo[row * 3 + 1] = uR; stereo[row * 3 + 2] = v;
  has_depth[row] = hd ? 1 : 0;
  if (kp_undist) { kp_undist[row * 3] = u; kp_undist[row * 3 + 1] = v; kp_undist[row * 3 + 2] = score; }
}

void launch_rgbd_associate(const float* kp, const int* lens, int frames, int max_kp, const void* depth, int depth_f32, int h, int w,
                           long long depth_stride, const RgbdK& c, float* kp_undist, float* stereo, uint8_t* has_depth, hipStream_t s) {
  hipLaunchKernelGGL(k_rgbd_associate, dim3((max_kp + 255) / 256, frames), dim3(256), 0, s, kp, lens, max_kp, depth, depth_f32, h, w,
                     depth_stride, c, kp_undist, stereo, has_depth);
}

}  // namespace sship
