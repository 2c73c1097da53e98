// Steered BRIEF descriptors and the Hamming matcher (include/sship.h "Binary descriptors", "Hamming matcher").  Integers and comparisons
// throughout (the gate's two fp32 subtractions apart): every output is a pure function of its inputs, and no kernel here has an atomic.
//
// k_brief_describe: one wave per keypoint, kBriefWaves keypoints per workgroup.  The wave stages the 33 x 33 patch into LDS with byte
//   loads (no alignment is asked of the image), forms the 33 x 29 horizontal 5-sums as u16 (a box sum is then five reads of one column),
//   takes the two moments over the disc by a wave reduction, lets lane k & 31 compute projection k and reduces to the lowest k of the
//   maximum, and then makes four 64-wide ballots of the comparisons: ballot q is output words 2q and 2q + 1.  The rotated table (32 KB of
//   int8) lies in device memory, one object for every wave; a wave reads 256 B of it per ballot, coalesced.
// k_hm_best: grid (row block, direction, pair).  A lane owns one row of the set its direction walks and keeps its 8 words in registers;
//   the workgroup streams the other set through LDS in tiles of kHmTile rows (with presence flags and, when gated, keypoints); every lane
//   reads the same LDS row (a broadcast), 8 xor + 8 popcount-accumulate, and keeps best / second best / index under strict < in ascending
//   index order: the smallest index wins a tie.
// k_hm_final: the mutual check and the three outputs.
#include "../../include/sship.h"
#include "brief_pattern.h"
#include "kernels.h"

namespace sship {

namespace {

constexpr BriefTable kBriefTableHost = make_brief_table();
static_assert(brief_table_reach(kBriefTableHost) == 14, "every rotated coordinate lies in [-14, 14]: reach 16 = 14 + the box half-width 2");
__device__ const BriefTable d_brief_table = make_brief_table();
struct BriefTrig { int c[kBriefBins], s[kBriefBins]; };
constexpr BriefTrig make_brief_trig() {
  BriefTrig t{};
  for (int k = 0; k < kBriefBins; ++k) { t.c[k] = kBriefCos[k]; t.s[k] = kBriefSin[k]; }
  return t;
}
__device__ const BriefTrig d_brief_trig = make_brief_trig();

constexpr int kBP = 2 * kBriefReach + 1;       // 33: the staged patch
constexpr int kBPitch = 36;                    // bytes per staged row
constexpr int kHsW = kBP - 4;                  // 29 horizontal 5-sums per row
constexpr int kHsPitch = 30;                   // u16 per row of them
constexpr int kMD = 2 * kBriefMomentRadius + 1;   // 31: the square around the moment disc
static_assert(kBriefMomentRadius < kBriefReach, "the moment disc lies inside the staged patch");

__device__ __forceinline__ bool brief_coord_ok(float x) { return x >= 0.f && x < 16384.f; }   // NaN and +-inf: false

}  // namespace

const BriefTable& brief_table_host() { return kBriefTableHost; }

template <bool STEER>
__global__ __launch_bounds__(kWave * kBriefWaves) void k_brief_describe(const uint8_t* __restrict__ imgs, long long image_stride, long long stride,
                                                                        int h, int w, const float* __restrict__ kp, const int* __restrict__ lens,
                                                                        int unit_stride, int K, uint32_t* __restrict__ desc,
                                                                        uint8_t* __restrict__ status, uint8_t* __restrict__ bin_out) {
  __shared__ uint8_t patch_s[kBriefWaves][kBP * kBPitch];
  __shared__ uint16_t hs_s[kBriefWaves][kBP * kHsPitch];
  const int img = blockIdx.y, wv = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  const int i = blockIdx.x * kBriefWaves + wv;
  const bool row = i < K;                          // wave-uniform; a wave without a row still meets the barriers
  const size_t unit = (size_t)img * unit_stride;
  uint8_t* patch = patch_s[wv];
  uint16_t* hs = hs_s[wv];
  int st = SSHIP_BRIEF_NONE, xa = 0, ya = 0;
  if (row) {
    const int n = min(max(lens[unit], 0), K);
    if (i < n) {
      const float* r = kp + (unit * K + i) * 3;
      const float x = r[0], y = r[1];
      st = SSHIP_BRIEF_BORDER;
      if (brief_coord_ok(x) && brief_coord_ok(y)) {
        xa = (int)floor((double)x + 0.5); ya = (int)floor((double)y + 0.5);
        if (xa - kBriefReach >= 0 && xa + kBriefReach < w && ya - kBriefReach >= 0 && ya + kBriefReach < h) st = SSHIP_BRIEF_OK;
      }
    }
  }
  const bool ok = st == SSHIP_BRIEF_OK;            // wave-uniform
  if (ok) {
    const uint8_t* src = imgs + (size_t)img * image_stride + (size_t)(ya - kBriefReach) * stride + (xa - kBriefReach);
    for (int idx = lane; idx < kBP * kBP; idx += kWave) {
      const int r = idx / kBP, c = idx - r * kBP;
      patch[r * kBPitch + c] = src[(size_t)r * stride + c];
    }
  }
  __syncthreads();
  int bin = 0;
  if (ok) {
    for (int idx = lane; idx < kBP * kHsW; idx += kWave) {
      const int r = idx / kHsW, c = idx - r * kHsW;
      const uint8_t* p = patch + r * kBPitch + c;
      hs[r * kHsPitch + c] = (uint16_t)(p[0] + p[1] + p[2] + p[3] + p[4]);
    }
    if (STEER) {
      int m10 = 0, m01 = 0;
      for (int idx = lane; idx < kMD * kMD; idx += kWave) {
        const int r = idx / kMD, c = idx - r * kMD, dy = r - kBriefMomentRadius, dx = c - kBriefMomentRadius;
        if (dx * dx + dy * dy <= kBriefMomentRadius * kBriefMomentRadius) {
          const int v = patch[(r + 1) * kBPitch + c + 1];
          m10 += dx * v; m01 += dy * v;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { m10 += __shfl_xor(m10, o, kWave); m01 += __shfl_xor(m01, o, kWave); }
      int bk = lane & (kBriefBins - 1);
      long long best = (long long)m10 * d_brief_trig.c[bk] + (long long)m01 * d_brief_trig.s[bk];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        const long long ov = __shfl_xor(best, o, kWave);
        const int ok_ = __shfl_xor(bk, o, kWave);
        if (ov > best || (ov == best && ok_ < bk)) { best = ov; bk = ok_; }
      }
      bin = bk;                                    // the same in every lane: both halves of the wave hold the 32 projections
    }
  }
  __syncthreads();
  if (!row) return;
  const size_t out_row = (size_t)img * K + i;
  uint32_t* d = desc + out_row * 8;
  if (ok) {
#pragma unroll
    for (int q = 0; q < kBriefBits / kWave; ++q) {
      const int8_t* t = d_brief_table.v[bin][q * kWave + lane];
      const int ax = t[0] + 14, ay = t[1] + 14, bx = t[2] + 14, by = t[3] + 14;   // the box's first row of 5-sums and its column
      int A = 0, B = 0;
#pragma unroll
      for (int r = 0; r < 5; ++r) { A += hs[(ay + r) * kHsPitch + ax]; B += hs[(by + r) * kHsPitch + bx]; }
      const unsigned long long m = __ballot(A < B);
      if (lane == 0) { d[2 * q] = (uint32_t)m; d[2 * q + 1] = (uint32_t)(m >> 32); }
    }
  } else if (lane < 8) {
    d[lane] = 0u;
  }
  if (lane == 0) {
    if (status) status[out_row] = (uint8_t)st;
    if (bin_out) bin_out[out_row] = (uint8_t)bin;
  }
}

void launch_brief_describe(const uint8_t* imgs, long long image_stride, int stride, int images, int h, int w, const float* kp, const int* lens,
                           int unit_stride, int max_kp, int mode, uint32_t* desc, uint8_t* status, uint8_t* bin, hipStream_t s) {
  const dim3 grid((max_kp + kBriefWaves - 1) / kBriefWaves, images), block(kWave * kBriefWaves);
  if (mode == SSHIP_BRIEF_STEERED)
    hipLaunchKernelGGL(k_brief_describe<true>, grid, block, 0, s, imgs, image_stride, (long long)stride, h, w, kp, lens, unit_stride, max_kp, desc,
                       status, bin);
  else
    hipLaunchKernelGGL(k_brief_describe<false>, grid, block, 0, s, imgs, image_stride, (long long)stride, h, w, kp, lens, unit_stride, max_kp, desc,
                       status, bin);
}

// ------------------------------------------------------------------------------------------------------
// the Hamming matcher
// ------------------------------------------------------------------------------------------------------
namespace {
constexpr int kHmAbsent = 0x7fffffff;             // above every distance (<= 256): "no such entry"
__device__ __forceinline__ bool hm_in_window(float x0, float y0, float x1, float y1, const float* g) {
  const float dx = x0 - x1, dy = y0 - y1;
  return dx >= g[0] && dx <= g[1] && dy >= g[2] && dy <= g[3];   // this form: a NaN coordinate is in no window
}
}  // namespace

// best [pairs][2][K]: fwd, then bwd; e1 [pairs][K]: the distance of fwd where it is >= 0
template <bool GATE>
__global__ __launch_bounds__(kHmRows) void k_hm_best(const int* __restrict__ lens, const uint32_t* __restrict__ desc,
                                                     const uint8_t* __restrict__ status, const float* __restrict__ kp, HmK c,
                                                     int* __restrict__ best, int* __restrict__ e1_out) {
  __shared__ uint4 tile[kHmTile][2];
  __shared__ float2 tile_kp[kHmTile];
  __shared__ int tile_ok[kHmTile];
  static_assert(kHmRows == 2 * kHmTile, "each thread stages one half row of the tile");
  const int pair = blockIdx.z, dir = blockIdx.y, K = c.max_kp, tid = threadIdx.x;
  const size_t u0 = (size_t)c.first0 + (size_t)pair * c.step0, u1 = (size_t)c.first1 + (size_t)pair * c.step1;
  const size_t ua = dir ? u1 : u0, ub = dir ? u0 : u1;   // a: the set whose rows the lanes own; b: the set that is streamed
  const int na = min(max(lens[ua], 0), K), nb = min(max(lens[ub], 0), K);
  const int r = blockIdx.x * kHmRows + tid;
  const bool mine = r < na && (!status || status[ua * K + r] == SSHIP_BRIEF_OK);
  uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
  float x = 0.f, y = 0.f;
  if (mine) {
    const uint4* p = reinterpret_cast<const uint4*>(desc + (ua * K + r) * 8);
    lo = p[0]; hi = p[1];
    if (GATE) { x = kp[(ua * K + r) * 3]; y = kp[(ua * K + r) * 3 + 1]; }
  }
  int e1 = kHmAbsent, e2 = kHmAbsent, j1 = -1;
  const int jr = tid >> 1, half = tid & 1;
  for (int j0 = 0; j0 < nb; j0 += kHmTile) {               // nb is the same for the whole workgroup
    __syncthreads();
    {
      const int j = j0 + jr;
      const bool in = j < nb;
      tile[jr][half] = in ? reinterpret_cast<const uint4*>(desc + (ub * K + j) * 8)[half] : make_uint4(0, 0, 0, 0);
      if (half == 0) {
        tile_ok[jr] = in && (!status || status[ub * K + j] == SSHIP_BRIEF_OK);
        if (GATE) tile_kp[jr] = in ? make_float2(kp[(ub * K + j) * 3], kp[(ub * K + j) * 3 + 1]) : make_float2(0.f, 0.f);
      }
    }
    __syncthreads();
    if (mine) {
      const int cnt = min(kHmTile, nb - j0);
      for (int jj = 0; jj < cnt; ++jj) {
        bool present = tile_ok[jj] != 0;
        if (GATE) {
          const float2 k = tile_kp[jj];
          present = present && (dir ? hm_in_window(k.x, k.y, x, y, c.gate) : hm_in_window(x, y, k.x, k.y, c.gate));   // dx = x0_i - x1_j in both
        }
        const uint4 a = tile[jj][0], b = tile[jj][1];
        int D = __popc(lo.x ^ a.x);
        D += __popc(lo.y ^ a.y); D += __popc(lo.z ^ a.z); D += __popc(lo.w ^ a.w);
        D += __popc(hi.x ^ b.x); D += __popc(hi.y ^ b.y); D += __popc(hi.z ^ b.z); D += __popc(hi.w ^ b.w);
        if (present) {
          if (D < e1) { e2 = e1; e1 = D; j1 = j0 + jj; }
          else if (D < e2) e2 = D;
        }
      }
    }
  }
  if (r < K) {
    bool pass = j1 >= 0;
    if (pass && c.max_distance != 0 && e1 > c.max_distance) pass = false;
    if (pass && c.ratio_percent != 0 && e2 != kHmAbsent && 100 * e1 > c.ratio_percent * e2) pass = false;
    best[((size_t)pair * 2 + dir) * K + r] = pass ? j1 : -1;
    if (dir == 0) e1_out[(size_t)pair * K + r] = pass ? e1 : -1;
  }
}

__global__ __launch_bounds__(256) void k_hm_final(const int* __restrict__ best, const int* __restrict__ e1_in, int K, int mutual,
                                                  int* __restrict__ matches0, int* __restrict__ dist0, float* __restrict__ mscores0) {
  const int pair = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K) return;
  const int* fwd = best + (size_t)pair * 2 * K;
  const int* bwd = fwd + K;
  const int f = fwd[i];                                   // -1 for a row >= n0 or without status OK
  const bool m = f >= 0 && (!mutual || bwd[f] == i);
  const int e1 = m ? e1_in[(size_t)pair * K + i] : -1;
  const size_t o = (size_t)pair * K + i;
  matches0[o] = m ? f : -1;
  dist0[o] = e1;
  if (mscores0) mscores0[o] = m ? (float)(256 - e1) * (1.f / 256.f) : 0.f;   // exact: an integer in [0, 256] times 2^-8
}

void launch_hm_match(const int* lens, const uint32_t* desc, const uint8_t* status, const float* kp, const HmK& c, int pairs, int* ws,
                     int* matches0, int* dist0, float* mscores0, hipStream_t s) {
  const int K = c.max_kp;
  int* best = ws;
  int* e1 = ws + (size_t)pairs * 2 * K;
  const dim3 grid((K + kHmRows - 1) / kHmRows, 2, pairs);
  if (c.gate_on) hipLaunchKernelGGL(k_hm_best<true>, grid, dim3(kHmRows), 0, s, lens, desc, status, kp, c, best, e1);
  else hipLaunchKernelGGL(k_hm_best<false>, grid, dim3(kHmRows), 0, s, lens, desc, status, kp, c, best, e1);
  hipLaunchKernelGGL(k_hm_final, dim3((K + 255) / 256, pairs), dim3(256), 0, s, best, e1, K, c.mutual, matches0, dist0, mscores0);
}

}  // namespace sship
