// RANSAC pose seed and inlier gate (include/sship.h "RANSAC pose seed and inlier gate"): hypothesise from three stereo
// correspondences, score every hypothesis against every present observation (MSAC), keep the best.
//   k_ransac_score   256-thread workgroups, grid (splits, pairs).  A workgroup compacts its pair's present observations into LDS once, in
//                    row order (X, uL, v, uR as fp32: 24 bytes each, and the compacted index of every sampleable one), then every lane
//                    owns ONE hypothesis at a time (h = chunk * 256 + tid, chunks strided over the pair's `splits` workgroups): it draws
//                    its three ranks, builds (R, t) and walks the observations.  All lanes read the same LDS address in the walk - a
//                    broadcast, no bank conflict - and a lane's cost is one running fp64 sum in row order: no cross-lane sum exists, so
//                    the summation order is the rule's by construction and a cost cannot depend on the partition or on the batch.  The
//                    workgroup's best (cost, h, pose) - a min, which has no rounding - goes to its record of the workspace.
//   k_ransac_finish  one workgroup per pair: the argmin over the pair's records (lower h on a tie), then the winner's inlier mask and
//                    the counts, one thread per eight rows.
// No floating-point contraction in this file: the rule rounds every product and sum once, which makes the device's (R, t) and costs the
// same operations as the fp64 restatement in tests/_ransac_ref.py.  No atomics.  No local array is indexed by a run-time value, so that
// nothing lives in scratch: profiles/ransac_resource_usage.txt.
#include <climits>

#include "../../include/sship.h"
#include "kernels.h"
#include "solver_math.h"

#pragma clang fp contract(off)

namespace sship {

namespace {

constexpr int kRansacThreads = 256;
constexpr int kRansacRows = kPoseMaxObs / kRansacThreads;  // 8 consecutive rows per thread when a pair is read
constexpr int kRansacScratch = 80;                         // bytes after the observations: 4 doubles, 4 ints, 8 ints

__host__ __device__ __forceinline__ size_t ransac_scratch_offset(int max_obs) { return ((size_t)max_obs * 26 + 15) & ~(size_t)15; }

__device__ __forceinline__ uint32_t ransac_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t ransac_u(uint32_t seed, uint32_t h, uint32_t j) {
  return ransac_mix(ransac_mix(seed + 0x9e3779b9u * (3u * h + j + 1u)));
}

// One row of a pair: its six floats, whether it is present and whether it is sampleable.
__device__ __forceinline__ void ransac_row(const float* __restrict__ points, const float* __restrict__ meas, const uint8_t* __restrict__ valid,
                                           size_t row, const RansacK& K, float* o, bool& present, bool& sampleable) {
  present = sampleable = false;
#pragma unroll
  for (int c = 0; c < 6; ++c) o[c] = 0.f;
  if (valid[row] == 0) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) { o[c] = points[row * 3 + c]; o[3 + c] = meas[row * 3 + c]; }
  bool p = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) p = p && solver_finitef(o[c]);
  present = p;
  sampleable = p && ((double)o[3] - (double)o[4] >= K.min_disparity);
}

// The orthonormal triad (e1, e2, e3 in E[0..2], E[3..5], E[6..8]) and the mean of three points; false when |n|^2 is not > min_area2.
__device__ __forceinline__ bool ransac_triad(const double* p0, const double* p1, const double* p2, double min_area2, double* E, double* mean) {
  const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
  const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
  const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const double nn = (nx * nx + ny * ny) + nz * nz;
  const double la = sqrt((ax * ax + ay * ay) + az * az), ln = sqrt(nn);
  E[0] = ax / la; E[1] = ay / la; E[2] = az / la;
  E[6] = nx / ln; E[7] = ny / ln; E[8] = nz / ln;
  E[3] = E[7] * E[2] - E[8] * E[1]; E[4] = E[8] * E[0] - E[6] * E[2]; E[5] = E[6] * E[1] - E[7] * E[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) mean[i] = ((p0[i] + p1[i]) + p2[i]) / 3.0;
  return nn > min_area2;
}

// One present observation at T (row-major [R | t]): its MSAC term, and whether it is an inlier.
__device__ __forceinline__ double ransac_term(const double* T, const RansacK& K, float Xx, float Xy, float Xz, float uL, float v, bool& in) {
  const double d0 = (double)Xx - T[3], d1 = (double)Xy - T[7], d2 = (double)Xz - T[11];
  const double x = (T[0] * d0 + T[4] * d1) + T[8] * d2;
  const double y = (T[1] * d0 + T[5] * d1) + T[9] * d2;
  const double z = (T[2] * d0 + T[6] * d1) + T[10] * d2;
  in = false;
  if (!(z > 0.0)) return K.thr2;
  const double iz = 1.0 / z;
  const double r0 = ((K.fx * x) * iz + K.cx) - (double)uL;
  const double r2 = ((K.fy * y) * iz + K.cy) - (double)v;
  const double e2 = r0 * r0 + r2 * r2;
  in = e2 < K.thr2;
  return in ? e2 : K.thr2;
}

}  // namespace

int ransac_splits(int num_hypotheses) {
  const int chunks = (num_hypotheses + kRansacThreads - 1) / kRansacThreads;
  return chunks < kRansacMaxSplits ? chunks : kRansacMaxSplits;
}
size_t ransac_workspace_bytes(int max_pairs, int num_hypotheses) {
  return (size_t)max_pairs * ransac_splits(num_hypotheses) * kRansacRecord * sizeof(double);
}

__global__ __launch_bounds__(kRansacThreads) void k_ransac_score(const float* __restrict__ points, const float* __restrict__ meas,
                                                                const uint8_t* __restrict__ valid, int max_obs, RansacK K,
                                                                double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* sA = reinterpret_cast<float4*>(smem);                                  // (X, uL) of compacted observation k
  float2* sB = reinterpret_cast<float2*>(smem + (size_t)max_obs * 16);           // (v, uR)
  uint16_t* sS = reinterpret_cast<uint16_t*>(smem + (size_t)max_obs * 24);       // rank -> compacted index
  char* scratch = smem + ransac_scratch_offset(max_obs);
  double* sWc = reinterpret_cast<double*>(scratch);                              // [4] a wave's best cost
  int* sWh = reinterpret_cast<int*>(scratch + 32);                               // [4] and its h
  int* sCnt = reinterpret_cast<int*>(scratch + 48);                              // [8] a wave's present and sampleable rows
  const int pair = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t base = (size_t)pair * max_obs;

  // ---- the pair's observations, compacted in row order ----
  float ob[kRansacRows][6];
  unsigned pres = 0, samp = 0;
#pragma unroll
  for (int k = 0; k < kRansacRows; ++k) {
    const int i = tid * kRansacRows + k;
    bool p = false, sm = false;
#pragma unroll
    for (int c = 0; c < 6; ++c) ob[k][c] = 0.f;
    if (i < max_obs) ransac_row(points, meas, valid, base + i, K, ob[k], p, sm);
    if (p) pres |= 1u << k;
    if (sm) samp |= 1u << k;
  }
  const int cP = __popc(pres), cS = __popc(samp);
  int iP = cP, iS = cS;   // inclusive scan over the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int tP = __shfl_up(iP, off, 64), tS = __shfl_up(iS, off, 64);
    if (lane >= off) { iP += tP; iS += tS; }
  }
  if (lane == 63) { sCnt[wave] = iP; sCnt[4 + wave] = iS; }
  __syncthreads();
  int offP = iP - cP, offS = iS - cS, nP = 0, m = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) { offP += sCnt[w]; offS += sCnt[4 + w]; }
    nP += sCnt[w]; m += sCnt[4 + w];
  }
#pragma unroll
  for (int k = 0; k < kRansacRows; ++k) {
    if (pres & (1u << k)) {   // offP < nP <= max_obs, offS < m <= nP
      sA[offP] = make_float4(ob[k][0], ob[k][1], ob[k][2], ob[k][3]);
      sB[offP] = make_float2(ob[k][5], ob[k][4]);
      if (samp & (1u << k)) { sS[offS] = (uint16_t)offP; ++offS; }
      ++offP;
    }
  }
  __syncthreads();

  // ---- one hypothesis per lane and chunk ----
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double bc = inf, bT[12];
  int bh = INT_MAX;
#pragma unroll
  for (int i = 0; i < 12; ++i) bT[i] = 0.0;
  const int H = K.num_hypotheses;
  for (int h0 = blockIdx.x * kRansacThreads; h0 < H; h0 += gridDim.x * kRansacThreads) {
    const int h = h0 + tid;
    if (h >= H || m < 3) continue;
    const uint32_t um = (uint32_t)m;
    uint32_t a = ransac_u(K.seed, (uint32_t)h, 0u) % um;
    uint32_t b = ransac_u(K.seed, (uint32_t)h, 1u) % (um - 1u);
    b += b >= a ? 1u : 0u;
    uint32_t c = ransac_u(K.seed, (uint32_t)h, 2u) % (um - 2u);
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    c += c >= lo ? 1u : 0u;
    c += c >= hi ? 1u : 0u;
    const int ia = sS[a], ib = sS[b], ic = sS[c];   // a, b, c < m
    double X[3][3], Y[3][3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int idx = s == 0 ? ia : (s == 1 ? ib : ic);
      const float4 A = sA[idx];
      const float2 B = sB[idx];
      X[s][0] = (double)A.x; X[s][1] = (double)A.y; X[s][2] = (double)A.z;
      const double uL = (double)A.w, v = (double)B.x, uR = (double)B.y;
      const double Z = K.fx * K.baseline / (uL - uR);
      Y[s][0] = (uL - K.cx) * Z / K.fx; Y[s][1] = (v - K.cy) * Z / K.fy; Y[s][2] = Z;
    }
    double EX[9], EY[9], mX[3], mY[3], T[12];
    bool ok = ransac_triad(X[0], X[1], X[2], K.min_area2, EX, mX);
    ok = ransac_triad(Y[0], Y[1], Y[2], K.min_area2, EY, mY) && ok;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        T[4 * i + j] = (EX[i] * EY[j] + EX[3 + i] * EY[3 + j]) + EX[6 + i] * EY[6 + j];
        ok = ok && solver_finite(T[4 * i + j]);
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      T[4 * i + 3] = mX[i] - ((T[4 * i] * mY[0] + T[4 * i + 1] * mY[1]) + T[4 * i + 2] * mY[2]);
      ok = ok && solver_finite(T[4 * i + 3]);
    }
    if (!ok) continue;
    double cost = 0.0;
#pragma unroll 4
    for (int k = 0; k < nP; ++k) {
      const float4 A = sA[k];
      const float v = sB[k].x;
      bool in;
      cost += ransac_term(T, K, A.x, A.y, A.z, A.w, v, in);
    }
    if (cost < bc) {   // chunks ascend in h: the lower h keeps a tie
      bc = cost; bh = h;
#pragma unroll
      for (int i = 0; i < 12; ++i) bT[i] = T[i];
    }
  }

  // ---- the workgroup's best: a min, the lower h on a tie ----
  double wc = bc;
  int wh = bh;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double oc = __shfl_xor(wc, off, 64);
    const int oh = __shfl_xor(wh, off, 64);
    if (oc < wc || (oc == wc && oh < wh)) { wc = oc; wh = oh; }
  }
  if (lane == 0) { sWc[wave] = wc; sWh[wave] = wh; }
  __syncthreads();
  wc = sWc[0]; wh = sWh[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const double oc = sWc[w];
    const int oh = sWh[w];
    if (oc < wc || (oc == wc && oh < wh)) { wc = oc; wh = oh; }
  }
  double* rec = partial + ((size_t)pair * gridDim.x + blockIdx.x) * kRansacRecord;
  if (wh == INT_MAX) {   // nothing scored here
    if (tid == 0) {
      rec[0] = inf; rec[1] = -1.0;
#pragma unroll
      for (int i = 0; i < 12; ++i) rec[2 + i] = 0.0;
    }
  } else if (bh == wh) {   // exactly one lane: every h belongs to one lane
    rec[0] = bc; rec[1] = (double)bh;
#pragma unroll
    for (int i = 0; i < 12; ++i) rec[2 + i] = bT[i];
  }
}

__global__ __launch_bounds__(kRansacThreads) void k_ransac_finish(const float* __restrict__ points, const float* __restrict__ meas,
                                                                 const uint8_t* __restrict__ valid, int max_obs, RansacK K,
                                                                 const double* __restrict__ partial, int splits, double* __restrict__ pose,
                                                                 int32_t* __restrict__ stats, double* __restrict__ cost,
                                                                 uint8_t* __restrict__ inlier) {
  __shared__ int s_cnt[4][3];
  const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t base = (size_t)pair * max_obs;
  const double* rec0 = partial + (size_t)pair * splits * kRansacRecord;
  double bc = __longlong_as_double(0x7ff0000000000000ll);
  int bh = -1, bs = 0;
  for (int s = 0; s < splits; ++s) {
    const double c = rec0[(size_t)s * kRansacRecord];
    const int h = (int)rec0[(size_t)s * kRansacRecord + 1];
    if (h >= 0 && (bh < 0 || c < bc || (c == bc && h < bh))) { bc = c; bh = h; bs = s; }
  }
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = bh >= 0 ? rec0[(size_t)bs * kRansacRecord + 2 + i] : ((i == 0 || i == 5 || i == 10) ? 1.0 : 0.0);
  int nP = 0, m = 0, nIn = 0;
#pragma unroll
  for (int k = 0; k < kRansacRows; ++k) {
    const int i = tid * kRansacRows + k;
    if (i >= max_obs) continue;
    float o[6];
    bool p, sm, in = false;
    ransac_row(points, meas, valid, base + i, K, o, p, sm);
    if (p && bh >= 0) (void)ransac_term(T, K, o[0], o[1], o[2], o[3], o[5], in);
    nP += p ? 1 : 0; m += sm ? 1 : 0; nIn += in ? 1 : 0;
    if (inlier) inlier[base + i] = in ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nP += __shfl_xor(nP, off, 64); m += __shfl_xor(m, off, 64); nIn += __shfl_xor(nIn, off, 64);
  }
  if (lane == 0) { s_cnt[wave][0] = nP; s_cnt[wave][1] = m; s_cnt[wave][2] = nIn; }
  __syncthreads();
  if (tid == 0) {
    nP = m = nIn = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { nP += s_cnt[w][0]; m += s_cnt[w][1]; nIn += s_cnt[w][2]; }
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[(size_t)pair * 12 + i] = T[i];
    stats[pair * 4 + 0] = nP; stats[pair * 4 + 1] = nIn; stats[pair * 4 + 2] = bh;
    stats[pair * 4 + 3] = bh >= 0 ? SSHIP_RANSAC_OK : (m < 3 ? SSHIP_RANSAC_TOO_FEW : SSHIP_RANSAC_NO_MODEL);
    cost[pair] = bc;
  }
}

void launch_ransac_solve(const float* points, const float* meas, const uint8_t* valid, int max_obs, int pairs, const RansacK& k,
                         void* workspace, double* pose, int32_t* stats, double* cost, uint8_t* inlier, hipStream_t s) {
  const int splits = ransac_splits(k.num_hypotheses);
  const size_t lds = ransac_scratch_offset(max_obs) + kRansacScratch;   // 53 328 bytes at max_obs = 2048
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(k_ransac_score, dim3(splits, pairs), dim3(kRansacThreads), lds, s, points, meas, valid, max_obs, k, partial);
  hipLaunchKernelGGL(k_ransac_finish, dim3(pairs), dim3(kRansacThreads), 0, s, points, meas, valid, max_obs, k, partial, splits, pose, stats,
                     cost, inlier);
}

}  // namespace sship
