// Pose-only stereo solver (include/sship.h "Pose-only stereo solver"): FrameTracker::track's objective (PoseOnlyStereoFactor
// under a Huber-robust diagonal noise) with the library's own Levenberg-Marquardt schedule, one 6x6 system per pair.
//   k_pose_solve   one 256-thread workgroup per pair, the whole LM loop inside the launch.  The observations are read once into
//                  registers (fp32, 8 per thread; 1 / sigma_uR as a double next to them); a trial is ONE pass over them that produces
//                  the cost, the 21 unique entries of H and the 6 of g together, all in fp64.  28 sums: per thread over its observations
//                  in index order, then a butterfly over the 64 lanes, then the 4 waves in wave order by thread 0 - one fixed order,
//                  and a workgroup sees nothing of the other pairs, so a pair's bits do not depend on the batch.  Thread 0 holds the
//                  state (T, H, g, c, lambda), solves the 6x6 Cholesky system, applies the SE(3) exponential (se3_retract,
//                  solver_math.h) and decides; the others wait at a barrier.  Two barriers per trial.  The grid is `pairs` workgroups,
//                  whatever the CU count.
//   k_pose_gather  one thread per keyframe keypoint: the observation list out of two frames' stereo points and matches0.
// No local array is indexed by a run-time value (every loop over the 8 observation slots and the 6x6 system is fully unrolled), so that
// nothing lives in scratch: profiles/pose_solve_resource_usage.txt.
#include "../../include/sship.h"
#include "kernels.h"
#include "solver_math.h"

namespace sship {

namespace {

constexpr int kPoseThreads = 256;
constexpr int kPoseSlots = kPoseMaxObs / kPoseThreads;  // 8
constexpr int kPoseSums = 28;                            // c, H (21, upper triangle by rows), g (6)

// One observation at pose T (row-major [R | t]): rho into acc[0], w J~^T J~ into acc[1..21], w J~^T r~ into acc[22..27].
__device__ __forceinline__ void pose_accumulate(const double* T, const PoseK& K, float Xx, float Xy, float Xz, float uL, float uR, float v,
                                                double inv_sigma_ur, double* acc) {
  const double d0 = (double)Xx - T[3], d1 = (double)Xy - T[7], d2 = (double)Xz - T[11];
  const double x = T[0] * d0 + T[4] * d1 + T[8] * d2;
  const double y = T[1] * d0 + T[5] * d1 + T[9] * d2;
  const double z = T[2] * d0 + T[6] * d1 + T[10] * d2;
  const double s0 = K.inv_sigma_px, s1 = inv_sigma_ur;
  if (!(z > 0.0)) {  // behind the camera: the constant residual, no gradient
    const double c2 = 2.0 * K.fx;
    const double r0 = c2 * s0, r1 = c2 * s1;
    const double e2 = r0 * r0 + r1 * r1 + r0 * r0;
    const double e = sqrt(e2);
    acc[0] += e <= K.k ? 0.5 * e2 : K.k * e - 0.5 * K.k2;
    return;
  }
  const double iz = 1.0 / z;
  const double xb = x - K.baseline;
  const double r0 = (K.fx * x * iz + K.cx - (double)uL) * s0;
  const double r1 = (K.fx * xb * iz + K.cx - (double)uR) * s1;
  const double r2 = (K.fy * y * iz + K.cy - (double)v) * s0;
  const double e2 = r0 * r0 + r1 * r1 + r2 * r2;
  const double e = sqrt(e2);
  const bool quad = e <= K.k;
  const double w = quad ? 1.0 : K.k / e;
  acc[0] += quad ? 0.5 * e2 : K.k * e - 0.5 * K.k2;
  // whitened gradients of the three residuals with respect to q: (a0, 0, a2) for uL and uR, (0, b1, b2) for v
  const double fiz = K.fx * iz, giz = K.fy * iz;
  const double a0 = fiz * s0, a2 = -fiz * x * iz * s0;
  const double c0 = fiz * s1, c2 = -fiz * xb * iz * s1;
  const double b1 = giz * s0, b2 = -giz * y * iz * s0;
  // rows of J~ = a^T [ [q]x | -I ]
  const double J[3][6] = {{-a2 * y, a2 * x - a0 * z, a0 * y, -a0, 0.0, -a2},
                          {-c2 * y, c2 * x - c0 * z, c0 * y, -c0, 0.0, -c2},
                          {b1 * z - b2 * y, b2 * x, -b1 * x, 0.0, -b1, -b2}};
  const double r[3] = {r0, r1, r2};
  int o = 1;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double wa0 = w * J[0][a], wa1 = w * J[1][a], wa2 = w * J[2][a];
#pragma unroll
    for (int b = a; b < 6; ++b) { acc[o] += wa0 * J[0][b] + wa1 * J[1][b] + wa2 * J[2][b]; ++o; }
    acc[22 + a] += wa0 * r[0] + wa1 * r[1] + wa2 * r[2];
  }
}

// (H + lambda I) delta = -g by Cholesky, H as the 21 upper-triangle entries by rows.  false: a pivot that is not > 0; the factorisation
// then runs on through sqrt and 1 / l of that pivot, so delta is undefined (NaN / Inf) and the caller must not use it.
__device__ __forceinline__ bool pose_solve6(const double* H, const double* g, double lambda, double* delta) {
  double A[6][6], L[6][6];
  int o = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) { A[b][a] = H[o] + (a == b ? lambda : 0.0); ++o; }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0)) ok = false;
    const double l = sqrt(d), il = 1.0 / l;
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s * il;
    }
  }
  double yv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * yv[k];
    yv[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = yv[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * delta[k];
    delta[i] = s / L[i][i];
  }
  return ok;
}

}  // namespace

__global__ __launch_bounds__(kPoseThreads) void k_pose_solve(const float* __restrict__ points, const float* __restrict__ meas,
                                                            const uint8_t* __restrict__ valid, const double* __restrict__ pose0, int max_obs,
                                                            PoseK K, double* __restrict__ pose, int32_t* __restrict__ stats,
                                                            double* __restrict__ cost, uint8_t* __restrict__ inlier) {
  __shared__ double s_T[12];                 // the pose every thread evaluates next
  __shared__ double s_red[4][kPoseSums];     // one row of sums per wave
  __shared__ int s_stop, s_count;
  const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t base = (size_t)pair * max_obs;

  // ---- the observations, once ----
  float ob[kPoseSlots][6];
  double isr[kPoseSlots];
  unsigned present = 0;
  if (tid == 0) s_count = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPoseSlots; ++k) {
    const int i = k * kPoseThreads + tid;
    bool p = false;
#pragma unroll
    for (int c = 0; c < 6; ++c) ob[k][c] = 0.f;
    isr[k] = 0.0;
    if (i < max_obs && valid[base + i] != 0) {
      const float* px = points + (base + i) * 3;
      const float* pm = meas + (base + i) * 3;
      p = true;
#pragma unroll
      for (int c = 0; c < 3; ++c) { ob[k][c] = px[c]; ob[k][3 + c] = pm[c]; }
#pragma unroll
      for (int c = 0; c < 6; ++c) p = p && solver_finitef(ob[k][c]);
      if (p) {
        const double d = fmax((double)ob[k][3] - (double)ob[k][4], 1e-3);
        const double q = K.d_cond / d;
        isr[k] = 1.0 / (K.sigma_d0 * sqrt(1.0 + q * q));
      }
    }
    if (p) present |= 1u << k;
  }
  if (present) atomicAdd(&s_count, __popc(present));
  // ---- the initial pose ----
  double T[12], H[21], g[6];
  double c = 0.0, c_init = 0.0, lambda = K.lambda0;
  int trials = 0, status = SSHIP_POSE_CONVERGED;
  bool done = false;
  if (tid == 0) {
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      T[i] = pose0 ? pose0[(size_t)pair * 12 + i] : ((i == 0 || i == 5 || i == 10) ? 1.0 : 0.0);
      fin = fin && solver_finite(T[i]);
      s_T[i] = T[i];
    }
    if (!fin) status = SSHIP_POSE_BAD_INPUT;
  }
  __syncthreads();
  const int n_obs = s_count;
  if (tid == 0) {
    if (status != SSHIP_POSE_BAD_INPUT && n_obs < 3) status = SSHIP_POSE_TOO_FEW;
    s_stop = status != SSHIP_POSE_CONVERGED;
  }
  __syncthreads();
  if (s_stop) {  // uniform: the pose out is the pose in
    if (inlier)
      for (int i = tid; i < max_obs; i += kPoseThreads) inlier[base + i] = 0;
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 12; ++i) pose[(size_t)pair * 12 + i] = T[i];
      stats[pair * 4 + 0] = n_obs; stats[pair * 4 + 1] = 0; stats[pair * 4 + 2] = 0; stats[pair * 4 + 3] = status;
      cost[pair * 2 + 0] = 0.0; cost[pair * 2 + 1] = 0.0;
    }
    return;
  }

  // ---- the LM loop: pass 0 evaluates T0, every later pass one trial pose ----
  bool first = true;
  for (;;) {
    // one pass at s_T
    double Tl[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Tl[i] = s_T[i];
    double acc[kPoseSums];
#pragma unroll
    for (int i = 0; i < kPoseSums; ++i) acc[i] = 0.0;
#pragma unroll
    for (int k = 0; k < kPoseSlots; ++k)
      if (present & (1u << k)) pose_accumulate(Tl, K, ob[k][0], ob[k][1], ob[k][2], ob[k][3], ob[k][4], ob[k][5], isr[k], acc);
#pragma unroll
    for (int i = 0; i < kPoseSums; ++i) {
      double v = acc[i];
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
      acc[i] = v;
    }
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kPoseSums; ++i) s_red[wave][i] = acc[i];
    }
    __syncthreads();
    if (tid == 0) {
      double S[kPoseSums];
#pragma unroll
      for (int i = 0; i < kPoseSums; ++i) S[i] = ((s_red[0][i] + s_red[1][i]) + s_red[2][i]) + s_red[3][i];
      bool take = false;  // S becomes the state
      if (first) {
        take = true; c_init = S[0];
      } else {
        const double cn = S[0];
        if (solver_finite(cn) && fabs(c - cn) <= fmax(K.abs_tol, K.rel_tol * c)) {
          take = true; done = true; status = SSHIP_POSE_CONVERGED;
        } else if (cn < c) {
          take = true; lambda /= 10.0;
        } else {
          lambda *= 10.0;
          if (lambda > K.lambda_max) { done = true; status = SSHIP_POSE_STALLED; }
        }
      }
      if (take) {
        c = S[0];
#pragma unroll
        for (int i = 0; i < 21; ++i) H[i] = S[1 + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] = S[22 + i];
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = Tl[i];
      }
      // the next trial pose, or the end
      while (!done) {
        if (trials >= K.max_iterations) { done = true; status = SSHIP_POSE_ITER_CAP; break; }
        double delta[6];
        const bool ok = pose_solve6(H, g, lambda, delta);
        ++trials;
        if (ok) {
          double Tn[12];
          se3_retract(T, delta, Tn);
#pragma unroll
          for (int i = 0; i < 12; ++i) s_T[i] = Tn[i];
          break;
        }
        lambda *= 10.0;
        if (lambda > K.lambda_max) { done = true; status = SSHIP_POSE_STALLED; }
      }
      if (done) {
#pragma unroll
        for (int i = 0; i < 12; ++i) s_T[i] = T[i];
      }
      s_stop = done;
    }
    first = false;
    __syncthreads();
    if (s_stop) break;
  }

  // ---- inliers at the final pose (s_T) ----
  if (tid == 0) s_count = 0;
  __syncthreads();
  {
    double Tl[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Tl[i] = s_T[i];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kPoseSlots; ++k) {
      const int i = k * kPoseThreads + tid;
      bool in = false;
      if (present & (1u << k)) {
        const double d0 = (double)ob[k][0] - Tl[3], d1 = (double)ob[k][1] - Tl[7], d2 = (double)ob[k][2] - Tl[11];
        const double x = Tl[0] * d0 + Tl[4] * d1 + Tl[8] * d2;
        const double y = Tl[1] * d0 + Tl[5] * d1 + Tl[9] * d2;
        const double z = Tl[2] * d0 + Tl[6] * d1 + Tl[10] * d2;
        if (z > 0.0) {
          const double iz = 1.0 / z;
          const double r0 = K.fx * x * iz + K.cx - (double)ob[k][3];
          const double r2 = K.fy * y * iz + K.cy - (double)ob[k][5];
          in = hypot(r0, r2) < K.inlier_px;
        }
      }
      cnt += in ? 1 : 0;
      if (inlier && i < max_obs) inlier[base + i] = in ? 1 : 0;
    }
    if (cnt) atomicAdd(&s_count, cnt);
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[(size_t)pair * 12 + i] = T[i];
    stats[pair * 4 + 0] = n_obs; stats[pair * 4 + 1] = s_count; stats[pair * 4 + 2] = trials; stats[pair * 4 + 3] = status;
    cost[pair * 2 + 0] = c_init; cost[pair * 2 + 1] = c;
  }
}

// One thread per keyframe keypoint of a pair; plain stores, every entry of the pair written.
__global__ __launch_bounds__(256) void k_pose_gather(const float* __restrict__ stereo0, const uint8_t* __restrict__ hd0,
                                                     const float* __restrict__ stereo1, const uint8_t* __restrict__ hd1,
                                                     const int32_t* __restrict__ matches0, const int* __restrict__ n0p, const int* __restrict__ n1p,
                                                     int n_stride, int R, PoseK K, float* __restrict__ points, float* __restrict__ meas,
                                                     uint8_t* __restrict__ valid) {
  const int pair = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  const int n0 = min(max(n0p[(size_t)pair * n_stride], 0), R), n1 = min(max(n1p[(size_t)pair * n_stride], 0), R);
  const size_t row = (size_t)pair * R + i;
  float X[3] = {0.f, 0.f, 0.f}, m[3] = {0.f, 0.f, 0.f};
  bool ok = false;
  if (i < n0) {
    const int j = matches0[row];
    if ((unsigned)j < (unsigned)n1) {  // 0 <= j < n1
      const size_t rj = (size_t)pair * R + j;
      ok = hd0[row] != 0 && hd1[rj] != 0;
      if (ok) {
        const double uL = stereo0[row * 3], uR = stereo0[row * 3 + 1], v = stereo0[row * 3 + 2];
        const double Z = K.fx * K.baseline / (uL - uR);
        X[0] = (float)((uL - K.cx) * Z / K.fx);
        X[1] = (float)((v - K.cy) * Z / K.fy);
        X[2] = (float)Z;
        m[0] = stereo1[rj * 3]; m[1] = stereo1[rj * 3 + 1]; m[2] = stereo1[rj * 3 + 2];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { points[row * 3 + c] = X[c]; meas[row * 3 + c] = m[c]; }
  valid[row] = ok ? 1 : 0;
}

void launch_pose_solve(const float* points, const float* meas, const uint8_t* valid, const double* pose0, int max_obs, int pairs,
                       const PoseK& k, double* pose, int32_t* stats, double* cost, uint8_t* inlier, hipStream_t s) {
  hipLaunchKernelGGL(k_pose_solve, dim3(pairs), dim3(kPoseThreads), 0, s, points, meas, valid, pose0, max_obs, k, pose, stats, cost, inlier);
}
void launch_pose_gather(const float* stereo0, const uint8_t* hd0, const float* stereo1, const uint8_t* hd1, const int32_t* matches0,
                        const int* n0, const int* n1, int n_stride, int max_obs, int pairs, const PoseK& k, float* points, float* meas,
                        uint8_t* valid, hipStream_t s) {
  hipLaunchKernelGGL(k_pose_gather, dim3((max_obs + 255) / 256, pairs), dim3(256), 0, s, stereo0, hd0, stereo1, hd1, matches0, n0, n1, n_stride,
                     max_obs, k, points, meas, valid);
}

}  // namespace sship
