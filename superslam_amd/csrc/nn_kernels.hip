// Mutual nearest-neighbour descriptor matcher (include/sship.h "Nearest-neighbour matcher"): hloc's NN-mutual / NN-ratio /
// NN-superpoint on the matrix cores.  One streaming pass over the two descriptor sets plus a finish; the fp32 [n0, n1] similarity matrix
// never reaches HBM.  The pass has the structure of the assignment's k_assign_stream (lg_kernels.hip): the 32 x 32 tiles of
// sim = d0 d1^T are computed in BOTH MFMA orientations, so that every statistic is lane-local:
//   acc_i = mfma(d1 tile, d0 tile): lane owns row i, its 16 registers are columns j  -> row top-2
//   acc_j = mfma(d0 tile, d1 tile): lane owns column j, its 16 registers are rows i  -> column top-2
// (the same products summed in the same k order: bit-identical values, which is what makes match(B, A) the exact inverse of match(A, B)).
// A statistic is a triple (best, argbest, second): the maximum, the SMALLEST index attaining it, and the maximum over all other entries -
// a duplicate of the best gives second == best.
#include "kernels.h"

namespace sship {

constexpr int kNnCh = 4;  // column chunks per row tile (blockIdx.z), as kAssignCh: 4x the waves, per-chunk row partials

struct Top2 {
  float best, second;
  int arg;
};
__device__ __forceinline__ Top2 top2_empty() { return Top2{-INFINITY, -INFINITY, 0x7fffffff}; }
// one more entry, indices offered in ASCENDING order (a later equal value never takes the arg-max; it becomes the second)
__device__ __forceinline__ void top2_push(Top2& t, float v, int idx) {
  const bool gt = v > t.best;
  const float lo = gt ? t.best : v;  // the loser of (best, v)
  t.second = lo > t.second ? lo : t.second;
  t.arg = gt ? idx : t.arg;
  t.best = gt ? v : t.best;
}
// merge of two triples over disjoint index sets: best = max, the smaller index wins ties, second = max(min(b_a, b_b), s_a, s_b)
__device__ __forceinline__ void top2_merge(Top2& t, float b, int a, float s) {
  const bool take = b > t.best || (b == t.best && a < t.arg);
  const float lo = b < t.best ? b : t.best;
  float sec = s > t.second ? s : t.second;
  sec = lo > sec ? lo : sec;
  t.arg = take ? a : t.arg;
  t.best = take ? b : t.best;
  t.second = sec;
}

// desc: [2 * pairs][R][256] fp16 (image 2p = set 0, 2p + 1 = set 1 of pair p; R = max_keypoints rows per image), lens [2 * pairs] read on
// the device and clamped to [0, R].  NP = R rounded up to 32 (tiles), NT = NP / 32.
// pcol_ba [pairs][NT][NP] float2 (best, arg) + pcol_s [pairs][NT][NP] (second): per (row tile, column) partials;
// prow_ba [pairs][kNnCh][NP] float2 + prow_s [pairs][kNnCh][NP]: per (column chunk, row) partials.
// Entries outside n0 x n1 are masked BY INDEX to -inf (rows >= n of a caller's buffer may hold anything); every address is clamped to the
// buffer's last row, so no lane reads outside it.
//
// kGate (k_nn_stream_gated; include/sship.h "Keypoint-window gate"): kp [2 * pairs][R][3] fp32 (x, y, score) and the gate (dx_lo, dx_hi, dy_lo,
// dy_hi).  An entry whose dx = x0_i - x1_j, dy = y0_i - y1_j is not inside the window is masked to -inf next to the index masking, in
// BOTH orientations from the same fp32 subtraction of the same two operands, so the row view and the column view of an entry agree.
// The column tile's 32 keypoints are staged next to its descriptors (two LDS slots, read where the descriptor fragments are read:
// before the loop's barrier); the wave's 32 row keypoints are staged once.  The 32 window tests of a lane are evaluated BEFORE the
// tile's MFMAs into one 32-bit mask (bit r: row-view register r, bit 16 + r: column-view register r), so that the keypoints do not
// occupy registers next to the accumulators.  Keypoint addresses are clamped like descriptor addresses.  The ungated instantiation
// compiles to the code it was before.
struct NnGate {
  float dx_lo, dx_hi, dy_lo, dy_hi;
};
__device__ __forceinline__ bool nn_in_window(float x0, float y0, float x1, float y1, const NnGate& g) {
  const float dx = x0 - x1, dy = y0 - y1;
  return dx >= g.dx_lo && dx <= g.dx_hi && dy >= g.dy_lo && dy <= g.dy_hi;  // this form: a NaN coordinate is in no window
}
template <bool kGate>
__device__ __forceinline__ float2* nn_kp_lds() {
  if constexpr (kGate) {
    __shared__ __attribute__((aligned(16))) float2 s_k[2 * 32 + 4 * 32];  // column-tile keypoints x 2 slots | row keypoints x 4 waves
    return s_k;
  } else {
    return nullptr;
  }
}
template <bool kGate>
__device__ __forceinline__ void nn_stream_body(const _Float16* __restrict__ desc, const int* __restrict__ lens, int R, int NP,
                                               float2* __restrict__ pcol_ba, float* __restrict__ pcol_s, float2* __restrict__ prow_ba,
                                               float* __restrict__ prow_s, const float* __restrict__ kp, NnGate g) {
  const int pair = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, jl = lane & 31, hh = lane >> 5;
  const int NT = NP >> 5, ti = blockIdx.x * 4 + wave, i0 = ti * 32;
  const int n0 = min(max(lens[2 * pair], 0), R), n1 = min(max(lens[2 * pair + 1], 0), R);
  if ((int)blockIdx.x * 128 >= n0) return;  // no row of this workgroup exists (uniform: before any barrier)
  const bool active = ti < NT && i0 < n0;   // wave-uniform: a wave past the end still stages column tiles and joins the barriers
  const _Float16* A = desc + ((size_t)(2 * pair) * R + min(i0 + jl, R - 1)) * 256 + hh * 8;
  const _Float16* Bm = desc + (size_t)(2 * pair + 1) * R * 256;
  h8_t fa[16];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) fa[ks] = *reinterpret_cast<const h8_t*>(A + ks * 16);
  const int my_i = i0 + jl;
  const int ro = 4 * hh;  // register r of this lane <-> tile-local index (r & 3) + 8 (r >> 2) + ro
  const int ntj_all = (n1 + 31) >> 5, per = (ntj_all + kNnCh - 1) / kNnCh;
  const int tj_lo = blockIdx.z * per, ntj = min(tj_lo + per, ntj_all);  // this workgroup's column tiles: [tj_lo, ntj)
  if (tj_lo >= ntj) return;
  // The four waves walk the same column tiles: a tile (32 rows x 512 B of set 1) is fetched once, coalesced, into a padded LDS buffer
  // (row stride 528 B: conflict-free ds_read_b128 fragments).  Two buffers; the next tile's loads are in flight during the MFMAs.
  constexpr int kRowH = 264;  // halfs per LDS row
  __shared__ __attribute__((aligned(16))) _Float16 s_b[2][32 * kRowH];
  typedef unsigned stg_t __attribute__((ext_vector_type(4)));
  stg_t stg[4];
  auto fetch = [&](int tj) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = threadIdx.x + 256 * q, row = u >> 5, unit = u & 31;
      stg[q] = *reinterpret_cast<const stg_t*>(Bm + (size_t)min(tj * 32 + row, R - 1) * 256 + unit * 8);
    }
  };
  auto put = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = threadIdx.x + 256 * q, row = u >> 5, unit = u & 31;
      *reinterpret_cast<stg_t*>(&s_b[buf][row * kRowH + unit * 8]) = stg[q];
    }
  };
  Top2 rowt = top2_empty();  // the lane's row over this chunk's columns (the two half-waves hold disjoint columns)
  // gated: wave 0 stages the column tile's keypoints (lane l: coordinate l & 1 of tile row l >> 1); every wave its own 32 row keypoints
  float2* const s_kc = nn_kp_lds<kGate>();
  float2* const s_kr = kGate ? s_kc + 2 * 32 + wave * 32 : nullptr;
  const float* K1 = kGate ? kp + (size_t)(2 * pair + 1) * R * 3 : nullptr;
  float stgk = 0.f, x0_me = 0.f, y0_me = 0.f;
  auto fetch_kp = [&](int tj) __attribute__((always_inline)) {
    if (wave == 0) stgk = K1[(size_t)min(tj * 32 + (lane >> 1), R - 1) * 3 + (lane & 1)];
  };
  auto put_kp = [&](int slot) __attribute__((always_inline)) {
    if (wave == 0) reinterpret_cast<float*>(s_kc + slot * 32)[lane] = stgk;
  };
  if constexpr (kGate) {
    const float* K0 = kp + (size_t)(2 * pair) * R * 3;
    reinterpret_cast<float*>(s_kr)[lane] = K0[(size_t)min(i0 + (lane >> 1), R - 1) * 3 + (lane & 1)];
    x0_me = K0[(size_t)min(i0 + jl, R - 1) * 3];
    y0_me = K0[(size_t)min(i0 + jl, R - 1) * 3 + 1];
    fetch_kp(tj_lo);
    put_kp(0);
  }
  fetch(tj_lo);
  put(0);
  __syncthreads();
  for (int tj = tj_lo; tj < ntj; ++tj) {
    const int j0 = tj * 32, buf = (tj - tj_lo) & 1;
    fetch(min(tj + 1, ntj - 1));  // unconditional (the last one re-reads this tile and is never used): keeps stg in registers
    if constexpr (kGate) fetch_kp(min(tj + 1, ntj - 1));
    const f16x_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f16x_t ai = zero16, aj = zero16;
    unsigned inwin = 0;  // gated: which of the lane's 32 entries of this tile are inside the window
    if constexpr (kGate) {
      if (active) {
        const float2* kc = s_kc + buf * 32;
        const float2 k1_me = kc[jl];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = (r & 3) + 8 * (r >> 2) + ro;
          const float2 k1 = kc[c], k0 = s_kr[c];
          inwin |= nn_in_window(x0_me, y0_me, k1.x, k1.y, g) ? 1u << r : 0u;              // (row my_i, column j0 + c)
          inwin |= nn_in_window(k0.x, k0.y, k1_me.x, k1_me.y, g) ? 1u << (16 + r) : 0u;  // (row i0 + c, column my_j)
        }
      }
    }
    if (active) {
      const _Float16* bt = &s_b[buf][jl * kRowH + hh * 8];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const h8_t fbk = *reinterpret_cast<const h8_t*>(bt + k * 16);
        ai = mfma32(fbk, fa[k], ai);
        aj = mfma32(fa[k], fbk, aj);
      }
    }
    put(buf ^ 1);  // the other buffer: its last readers passed the barrier at the end of the previous iteration
    if constexpr (kGate) put_kp(buf ^ 1);
    __syncthreads();
    if (!active) continue;
    const int my_j = j0 + jl;
    // entries outside n0 x n1 become -inf; only the last row tile / column tile can have any (wave-uniform branches)
    if (j0 + 32 > n1) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (j0 + (r & 3) + 8 * (r >> 2) + ro >= n1) ai[r] = -INFINITY;
      if (my_j >= n1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) aj[r] = -INFINITY;
      }
    }
    if (i0 + 32 > n0) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (i0 + (r & 3) + 8 * (r >> 2) + ro >= n0) aj[r] = -INFINITY;
      if (my_i >= n0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) ai[r] = -INFINITY;
      }
    }
    // gated: entries outside the keypoint window become -inf too (absent, like the ones above)
    if constexpr (kGate) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (!(inwin >> r & 1u)) ai[r] = -INFINITY;
        if (!(inwin >> (16 + r) & 1u)) aj[r] = -INFINITY;
      }
    }
    // ---- row: the lane's 16 columns of this tile, ascending j
#pragma unroll
    for (int r = 0; r < 16; ++r) top2_push(rowt, ai[r], j0 + (r & 3) + 8 * (r >> 2) + ro);
    // ---- column partial over the 32 rows of this wave: the lane's 16 rows, ascending i, then the other half-wave's
    Top2 colt = top2_empty();
#pragma unroll
    for (int r = 0; r < 16; ++r) top2_push(colt, aj[r], i0 + (r & 3) + 8 * (r >> 2) + ro);
    top2_merge(colt, __shfl_xor(colt.best, 32, 64), __shfl_xor(colt.arg, 32, 64), __shfl_xor(colt.second, 32, 64));
    if (hh == 0 && my_j < n1) {
      const size_t o = ((size_t)pair * NT + ti) * NP + my_j;
      pcol_ba[o] = make_float2(colt.best, __int_as_float(colt.arg));
      pcol_s[o] = colt.second;
    }
  }
  if (!active) return;
  top2_merge(rowt, __shfl_xor(rowt.best, 32, 64), __shfl_xor(rowt.arg, 32, 64), __shfl_xor(rowt.second, 32, 64));
  if (hh == 0 && my_i < n0) {
    const size_t o = ((size_t)pair * kNnCh + blockIdx.z) * NP + my_i;
    prow_ba[o] = make_float2(rowt.best, __int_as_float(rowt.arg));
    prow_s[o] = rowt.second;
  }
}

__global__ __launch_bounds__(256, 2) void k_nn_stream(const _Float16* __restrict__ desc, const int* __restrict__ lens, int R, int NP,
                                                      float2* __restrict__ pcol_ba, float* __restrict__ pcol_s,
                                                      float2* __restrict__ prow_ba, float* __restrict__ prow_s) {
  nn_stream_body<false>(desc, lens, R, NP, pcol_ba, pcol_s, prow_ba, prow_s, nullptr, NnGate{});
}
__global__ __launch_bounds__(256, 2) void k_nn_stream_gated(const _Float16* __restrict__ desc, const int* __restrict__ lens, int R, int NP,
                                                            float2* __restrict__ pcol_ba, float* __restrict__ pcol_s,
                                                            float2* __restrict__ prow_ba, float* __restrict__ prow_s,
                                                            const float* __restrict__ kp, NnGate g) {
  nn_stream_body<true>(desc, lens, R, NP, pcol_ba, pcol_s, prow_ba, prow_s, kp, g);
}

// folds of the partials in ascending part order (max / min only: any order gives the same triple)
__device__ __forceinline__ Top2 nn_fold(const float2* ba, const float* sec, int nparts, int NP) {
  Top2 t = top2_empty();
  for (int k = 0; k < nparts; ++k) {
    const float2 v = ba[(size_t)k * NP];
    top2_merge(t, v.x, __float_as_int(v.y), sec[(size_t)k * NP]);
  }
  return t;
}
// the ratio and distance tests on e = 2 (1 - sim), the squared L2 distance of unit rows (include/sship.h); `single`: no second exists
__device__ __forceinline__ bool nn_pass(float s1, float s2, bool single, float ratio, float dist) {
  const float e1 = 2.f * (1.f - s1), e2 = 2.f * (1.f - s2);
  const bool rt = !(ratio > 0.f) || single || e1 <= (ratio * ratio) * e2;
  const bool dt = !(dist > 0.f) || e1 <= dist * dist;
  return rt && dt;
}
// One thread per row: row i's top-2 (folded over the column chunks), the tests, and - with the mutual check - column j1's top-2 (folded
// over the row tiles), the same tests there, and bwd[j1] == i.  Writes all max_kp entries of the pair: rows >= n0 are -1 / 0.
// kGate: "no second exists" is read off the statistic itself - second == -inf means fewer than two entries of the row / column were
// present (an absent entry is -inf, a present one is a finite sum) - instead of off the count; a row with no present entry keeps
// arg = 0x7fffffff and fails the bounds check.
template <bool kGate>
__device__ __forceinline__ void nn_final_body(const float2* __restrict__ pcol_ba, const float* __restrict__ pcol_s,
                                              const float2* __restrict__ prow_ba, const float* __restrict__ prow_s,
                                              const int* __restrict__ lens, int R, int NP, float ratio, float dist, int mutual,
                                              int32_t* __restrict__ matches0, float* __restrict__ mscores0) {
  const int pair = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  const int n0 = min(max(lens[2 * pair], 0), R), n1 = min(max(lens[2 * pair + 1], 0), R);
  const int NT = NP >> 5;
  int mj = -1;
  float ms = 0.f;
  if (i < n0 && n1 > 0) {
    const int ntj_all = (n1 + 31) >> 5, per = (ntj_all + kNnCh - 1) / kNnCh;
    const size_t ro = (size_t)pair * kNnCh * NP + i;
    const Top2 rt = nn_fold(prow_ba + ro, prow_s + ro, (ntj_all + per - 1) / per, NP);
    const int j1 = rt.arg;
    bool ok = (unsigned)j1 < (unsigned)n1 && nn_pass(rt.best, rt.second, kGate ? rt.second == -INFINITY : n1 == 1, ratio, dist);
    if (ok && mutual) {
      const size_t co = (size_t)pair * NT * NP + j1;
      const Top2 ct = nn_fold(pcol_ba + co, pcol_s + co, (n0 + 31) >> 5, NP);
      ok = ct.arg == i && nn_pass(ct.best, ct.second, kGate ? ct.second == -INFINITY : n0 == 1, ratio, dist);
    }
    if (ok) { mj = j1; ms = rt.best; }
  }
  matches0[(size_t)pair * R + i] = mj;
  mscores0[(size_t)pair * R + i] = ms;
}
__global__ __launch_bounds__(256) void k_nn_final(const float2* __restrict__ pcol_ba, const float* __restrict__ pcol_s,
                                                  const float2* __restrict__ prow_ba, const float* __restrict__ prow_s,
                                                  const int* __restrict__ lens, int R, int NP, float ratio, float dist, int mutual,
                                                  int32_t* __restrict__ matches0, float* __restrict__ mscores0) {
  nn_final_body<false>(pcol_ba, pcol_s, prow_ba, prow_s, lens, R, NP, ratio, dist, mutual, matches0, mscores0);
}
__global__ __launch_bounds__(256) void k_nn_final_gated(const float2* __restrict__ pcol_ba, const float* __restrict__ pcol_s,
                                                        const float2* __restrict__ prow_ba, const float* __restrict__ prow_s,
                                                        const int* __restrict__ lens, int R, int NP, float ratio, float dist, int mutual,
                                                        int32_t* __restrict__ matches0, float* __restrict__ mscores0) {
  nn_final_body<true>(pcol_ba, pcol_s, prow_ba, prow_s, lens, R, NP, ratio, dist, mutual, matches0, mscores0);
}

// StereoFrontEnd::process's association (include/sship.h "Stereo association"): one thread per left keypoint of a pair, plain stores, every
// entry of the pair written.  kp [2 * pairs][R][3], lens [2 * pairs] clamped to [0, R], matches0 [pairs][R] (either matcher's).
__global__ __launch_bounds__(256) void k_stereo_associate(const float* __restrict__ kp, const int* __restrict__ lens,
                                                          const int32_t* __restrict__ matches0, int R, float min_disparity,
                                                          float max_row_diff, float* __restrict__ stereo, uint8_t* __restrict__ has_depth) {
  const int pair = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  const int n0 = min(max(lens[2 * pair], 0), R), n1 = min(max(lens[2 * pair + 1], 0), R);
  float uL = 0.f, vL = 0.f, uR = __builtin_nanf("");
  bool hd = false;
  if (i < n0) {
    const float* kl = kp + ((size_t)(2 * pair) * R + i) * 3;
    uL = kl[0]; vL = kl[1];
    const int j = matches0[(size_t)pair * R + i];
    if ((unsigned)j < (unsigned)n1) {  // 0 <= j < n1
      const float* kr = kp + ((size_t)(2 * pair + 1) * R + j) * 3;
      const float u = kr[0], v = kr[1];
      hd = (uL - u >= min_disparity) && (fabsf(vL - v) <= max_row_diff);  // the positive form: NaN gives no depth
      if (hd) uR = u;
    }
  }
  float* o = stereo + ((size_t)pair * R + i) * 3;
  o[0] = uL; o[1] = uR; o[2] = vL;
  has_depth[(size_t)pair * R + i] = hd ? 1 : 0;
}

size_t nn_workspace_floats(int max_kp, int max_pairs) {
  const size_t NP = (size_t)(max_kp + 31) / 32 * 32, NT = NP / 32;
  return (size_t)max_pairs * (NT + kNnCh) * NP * 3;
}
void launch_nn_match(const _Float16* desc, const int* lens, int max_kp, int pairs, float* ws, float ratio, float dist, int mutual,
                     int32_t* matches0, float* mscores0, hipStream_t s) {
  const int NP = (max_kp + 31) / 32 * 32, NT = NP / 32;
  // ws: pcol_ba [P][NT][NP][2] | prow_ba [P][kNnCh][NP][2] | pcol_s [P][NT][NP] | prow_s [P][kNnCh][NP]
  float2* pcol_ba = reinterpret_cast<float2*>(ws);
  float2* prow_ba = pcol_ba + (size_t)pairs * NT * NP;
  float* pcol_s = reinterpret_cast<float*>(prow_ba + (size_t)pairs * kNnCh * NP);
  float* prow_s = pcol_s + (size_t)pairs * NT * NP;
  hipLaunchKernelGGL(k_nn_stream, dim3((NT + 3) / 4, pairs, kNnCh), dim3(256), 0, s, desc, lens, max_kp, NP, pcol_ba, pcol_s, prow_ba, prow_s);
  hipLaunchKernelGGL(k_nn_final, dim3((max_kp + 255) / 256, pairs), dim3(256), 0, s, pcol_ba, pcol_s, prow_ba, prow_s, lens, max_kp, NP,
                     ratio, dist, mutual, matches0, mscores0);
}

void launch_nn_match_gated(const _Float16* desc, const float* kp, const int* lens, int max_kp, int pairs, float* ws, float ratio, float dist,
                           int mutual, const float gate[4], int32_t* matches0, float* mscores0, hipStream_t s) {
  const int NP = (max_kp + 31) / 32 * 32, NT = NP / 32;
  float2* pcol_ba = reinterpret_cast<float2*>(ws);  // the layout of launch_nn_match
  float2* prow_ba = pcol_ba + (size_t)pairs * NT * NP;
  float* pcol_s = reinterpret_cast<float*>(prow_ba + (size_t)pairs * kNnCh * NP);
  float* prow_s = pcol_s + (size_t)pairs * NT * NP;
  const NnGate g{gate[0], gate[1], gate[2], gate[3]};
  hipLaunchKernelGGL(k_nn_stream_gated, dim3((NT + 3) / 4, pairs, kNnCh), dim3(256), 0, s, desc, lens, max_kp, NP, pcol_ba, pcol_s, prow_ba,
                     prow_s, kp, g);
  hipLaunchKernelGGL(k_nn_final_gated, dim3((max_kp + 255) / 256, pairs), dim3(256), 0, s, pcol_ba, pcol_s, prow_ba, prow_s, lens, max_kp, NP,
                     ratio, dist, mutual, matches0, mscores0);
}
void launch_stereo_associate(const float* kp, const int* lens, const int32_t* matches0, int max_kp, int pairs, float min_disparity,
                             float max_row_diff, float* stereo, uint8_t* has_depth, hipStream_t s) {
  hipLaunchKernelGGL(k_stereo_associate, dim3((max_kp + 255) / 256, pairs), dim3(256), 0, s, kp, lens, matches0, max_kp, min_disparity,
                     max_row_diff, stereo, has_depth);
}

}  // namespace sship
